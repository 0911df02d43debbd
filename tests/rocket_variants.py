"""Variants of tests/golden/rocket_mini.config by text replacement, shared by the rocket_launching tests; the synthetic batches are
examples/train_from_config.py's (a sample weight column when the config names one)."""
import os

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "rocket_mini.config")).read()

SHARE = "        share_mlp { hidden_units: [24] }\n"
BOOSTER = "        booster_mlp { hidden_units: [32, 16, 8] }\n"
LIGHT = "        light_mlp { hidden_units: [16, 8] }\n"
FLAG = "        feature_based_distillation: true\n"
FUNCTION = "        feature_distillation_function: COSINE\n"
WEIGHTS = '    sample_weight_fields: "weight"\n'
CLASSES = "    num_class: 1\n"
LOSSES = "    losses { binary_cross_entropy {} }\n"

NAMES = ("mini", "no_share", "two_class", "distance", "no_weights", "flag_off")


def swap(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def variant(name, text=TEXT):
    """mini: the file; no_share: no share MLP; two_class: num_class 2 with softmax_cross_entropy (and so no weights: the model
    refuses the two together); distance: INNER_PRODUCT, the reference's `else` branch; no_weights; flag_off: no feature based
    distillation, the hint loss alone"""
    if name == "mini":
        return text
    if name == "no_share":
        return swap(text, SHARE, "")
    if name == "two_class":
        text = swap(swap(text, CLASSES, "    num_class: 2\n"), LOSSES, "    losses { softmax_cross_entropy {} }\n")
        return swap(text, WEIGHTS, "")
    if name == "distance":
        return swap(text, FUNCTION, "        feature_distillation_function: INNER_PRODUCT\n")
    if name == "no_weights":
        return swap(text, WEIGHTS, "")
    if name == "flag_off":
        return swap(text, FLAG, "        feature_based_distillation: false\n")
    raise KeyError(name)


def batches(spec, B, n, seed=0):
    """n host batches of B rows"""
    from examples.train_from_config import synthetic_batches

    return list(synthetic_batches(spec, B * n, B, seed=seed))
