"""The library's kind table (torcheasyrec_amd/opt_kinds.py) against the tests' own numpy references, which stay independent
of it: the two must agree on how wide a kind's state row is."""
import os
import sys

import pytest

HERE = os.path.dirname(__file__)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import sparse_optim_elem_ref  # noqa: E402
import sparse_optim_ref  # noqa: E402
from torcheasyrec_amd import _lib, opt_kinds  # noqa: E402


@pytest.mark.parametrize("kind", sorted(opt_kinds.KINDS))
def test_state_width_agrees_with_the_references(kind):
    ref = sparse_optim_elem_ref if kind in ("adadelta", "rmsprop") else sparse_optim_ref
    for D in (4, 16, 20, 64, 128, 256):
        assert opt_kinds.KINDS[kind].state_width(D) == ref.state_width(kind, D), (kind, D)
    assert opt_kinds.KINDS[kind].code == getattr(_lib, "OPT_" + kind.upper())  # (opt_kinds spells the codes out: no torch import)
