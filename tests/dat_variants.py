"""Variants of tests/golden/dat_mini.config by text replacement, shared by the dat tests; the synthetic batches are the dssm
tests' (tests/dssm_variants.py: user-side features in the base data group, item-side ones in "__NEG__" under a sampler)."""
import os

from dssm_variants import batches, with_line  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "dat_mini.config")).read()

SAMPLER = TEXT[TEXT.index("    negative_sampler {"):TEXT.index("        item_id_field: \"adgroup_id\"\n    }\n") + len("        item_id_field: \"adgroup_id\"\n    }\n")]
WEIGHTS_ANCHOR, WEIGHTS_LINE = '    label_fields: "clk"\n', '    sample_weight_fields: "w"\n'


def in_batch(text=TEXT):
    """no sampler, `in_batch_negative: true`: the other rows of the batch are the negatives"""
    assert text.count(SAMPLER) == 1 and text.count("        temperature: 0.05\n") == 1
    return text.replace(SAMPLER, "").replace("        temperature: 0.05\n", "        temperature: 0.05\n        in_batch_negative: true\n")


def variant(name, weights=False, text=TEXT):
    text = text if name == "sampled" else in_batch(text)
    return with_line(text, WEIGHTS_ANCHOR, WEIGHTS_LINE) if weights else text


def amm_weights(text, u, i):
    assert text.count("        amm_i_weight: 0.5\n        amm_u_weight: 0.5\n") == 1
    return text.replace("        amm_i_weight: 0.5\n        amm_u_weight: 0.5\n", f"        amm_i_weight: {i}\n        amm_u_weight: {u}\n")
