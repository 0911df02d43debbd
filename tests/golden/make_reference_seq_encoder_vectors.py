"""Generate tests/golden/reference_seq_encoder_vectors.npz by RUNNING the reference's own SimpleAttention and PoolingEncoder
(tzrec/modules/sequence.py:131-218) on the CPU in fp32.  Needs the reference checkout that make_reference_module_vectors.py
imports from (same import shim); the tests need only the .npz:

    python tests/golden/make_reference_seq_encoder_vectors.py

Cases: B = 6, L = 8, lengths [0, 1, 3, 8, 8, 5], D in {16, 48}, max_seq_length in {0, 6}; the rows behind a sample's length
are zero, as to_padded_dense leaves them.  Stored per case: query, sequence, length, output, a fixed output gradient and the
input gradients autograd gives for it."""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

LENGTHS = [0, 1, 3, 8, 8, 5]
B, L = 6, 8


def main():
    install_reference_imports()
    seq_mod = importlib.import_module("tzrec.modules.sequence")
    torch.manual_seed(20261017)
    torch.set_num_threads(1)
    out = {}
    ln = torch.tensor(LENGTHS, dtype=torch.int64)
    for D in (16, 48):
        for msl in (0, 6):
            encoders = {"attn": seq_mod.SimpleAttention(sequence_dim=D, query_dim=D, input="g", max_seq_length=msl),
                        "sum": seq_mod.PoolingEncoder(sequence_dim=D, input="g", pooling_type="sum", max_seq_length=msl),
                        "mean": seq_mod.PoolingEncoder(sequence_dim=D, input="g", pooling_type="mean", max_seq_length=msl)}
            for kind, enc in encoders.items():
                tag = f"{kind}_d{D}_m{msl}"
                q = torch.randn(B, D, requires_grad=True)
                s = (torch.randn(B, L, D) * (torch.arange(L).unsqueeze(0) < ln.unsqueeze(1)).unsqueeze(2)).requires_grad_(True)
                y = enc({"g.query": q, "g.sequence": s, "g.sequence_length": ln})
                gy = torch.randn_like(y)
                y.backward(gy)
                out[f"{tag}/query"], out[f"{tag}/sequence"], out[f"{tag}/length"] = _np(q), _np(s), _np(ln)
                out[f"{tag}/y"], out[f"{tag}/gy"], out[f"{tag}/gsequence"] = _np(y), _np(gy), _np(s.grad)
                if kind == "attn":
                    out[f"{tag}/gquery"] = _np(q.grad)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_seq_encoder_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
