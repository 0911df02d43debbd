"""Variants of tests/golden/dbmtl_mini.config by text replacement, shared by the dbmtl tests."""
import os

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "dbmtl_mini.config")).read()

SEQ_FEATURES = """feature_configs {
    sequence_feature {
        sequence_name: "click_seq"
        sequence_length: 8
        sequence_delim: "|"
        features { id_feature { feature_name: "adgroup_id" num_buckets: 300 embedding_dim: 16 } }
        features { id_feature { feature_name: "cate_id" num_buckets: 40 embedding_dim: 16 } }
    }
}
"""
SEQ_BLOCKS = """        sequence_groups {
            group_name: "click_seq"
            feature_names: "adgroup_id"
            feature_names: "cate_id"
            feature_names: "click_seq__adgroup_id"
            feature_names: "click_seq__cate_id"
        }
        sequence_encoders { din_encoder { attn_mlp { hidden_units: [8, 4] } } }
"""


def with_sequence(text=TEXT):
    """the `dbmtl_has_sequence` style: a click history as a nested sequence group of the DEEP group, reduced by a din_encoder
    (the blocks of tests/golden/mmoe_seq_mini.config)"""
    assert text.count("model_config {\n") == 1 and text.count("        group_type: DEEP\n") == 1
    return text.replace("model_config {\n", SEQ_FEATURES + "model_config {\n").replace("        group_type: DEEP\n", "        group_type: DEEP\n" + SEQ_BLOCKS)
