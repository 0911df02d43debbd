"""The `*_ok` / `*_supported` predicates of the fused ops: which row operands each one takes.

One table of [rows, cols] tensors -- the layouts tests/test_operands.py holds `_lib.rows_ok` to -- is put into every row operand
position of every predicate, all other operands valid, at the smallest legal shapes (B = 3, D = H = 8, M = 5, K = 2, S = 4, one
pair, one slot, two towers of one layer; the tall-input linears at their smallest built shape, K = 16, H = 64).  What is
expected is what the predicate's docstring says, by class of predicate:

* F4: the float4 row rule of tzr_rows_operand -- contiguous rows and a 16-byte aligned column slice pass, nothing else does;
* LEADING: the tall-input linears read the leading K columns of fp32 rows with unit column stride, a row stride that is a
  multiple of 4 floats and 16-byte aligned data; their docstrings ask for no more (the library checks the row stride against K);
* SKINNY_W: the weight of a skinny Linear: fp32, unit column stride, a row stride that is a multiple of 4 floats (no docstring:
  the rule as written);
* ANY: operands the op copies itself where it must (`rows16` / `scalar_rows` in its forward): every fp32 2-D layout passes.

fp64, fp16 and 1-D operands are refused everywhere.  Then per predicate one case on the wrong device for the loaded library and
one with a malformed weights (bias, initial logits) vector."""
import pytest
import torch

from torcheasyrec_amd import capsule, dense, gate_ops, masknet, match, rocket, wukong

LAYOUTS = ("contiguous", "column_slice", "misaligned", "row_stride_odd", "expanded", "transposed", "one_row")
REFUSED = ("fp64", "fp16", "one_dim")


def _entry(name, rows, cols, dev):
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    if name == "contiguous":
        return z(rows, cols)
    if name == "column_slice":
        return z(rows, 2 * cols)[:, 4:4 + cols]
    if name == "misaligned":
        return z(rows, 2 * cols)[:, 1:1 + cols]
    if name == "row_stride_odd":  # cols + 2 floats: no multiple of 4 at any width used here
        return z(rows, cols + 2)[:, :cols]
    if name == "expanded":
        return z(1, cols).expand(rows, cols)
    if name == "transposed":
        return z(cols, rows).t()
    if name == "one_row":  # rows == 1: row stride cols + 2, first float 8 bytes past a 16-byte boundary
        assert rows == 1 and (cols + 2) * 4 % 16 == 8
        return z(4, cols + 2)[1:2, :cols]
    if name == "fp64":
        return z(rows, cols).double()
    if name == "fp16":
        return z(rows, cols).half()
    assert name == "one_dim"
    return z(cols)


F4 = {"contiguous", "column_slice"}
LEADING = {"contiguous", "column_slice", "expanded"}
SKINNY_W = {"contiguous", "column_slice", "misaligned", "expanded"}
ANY = set(LAYOUTS)


def _match(dev, B, M):
    o = {"user": torch.zeros(B, 8, device=dev), "item": torch.zeros(M, 8, device=dev), "weights": None}
    return o, lambda o: match.match_softmax_ok(o["user"], o["item"], match.SAMPLED, o["weights"])


def _label_attention(dev, B, M):
    o = {"interests": torch.zeros(B, 2, 8, device=dev), "item": torch.zeros(M, 8, device=dev),
         "mask": torch.ones(B, 2, dtype=torch.bool, device=dev)}
    return o, lambda o: match.label_attention_ok(o["interests"], o["item"], o["mask"], 1.0)


def _amm(dev, B, M):
    o = {"user_aug": torch.zeros(B, 8, device=dev), "item_aug": torch.zeros(M, 8, device=dev), "user_emb": torch.zeros(B, 8, device=dev),
         "item_emb": torch.zeros(M, 8, device=dev), "weights": None}
    return o, lambda o: match.amm_loss_ok(o["user_aug"], o["item_aug"], o["user_emb"], o["item_emb"], o["weights"])


def _distill(dev, B, M):
    o = {"light": torch.zeros(B, 8, device=dev), "booster": torch.zeros(B, 8, device=dev), "logits_light": torch.zeros(B, device=dev),
         "logits_booster": torch.zeros(B, device=dev), "weights": None}
    return o, lambda o: rocket.distill_losses_ok([o["light"]], [o["booster"]], o["logits_light"], o["logits_booster"], o["weights"])


def _capsule(dev, B, M):
    cfg = capsule.CapsuleConfig(max_k=2, max_seq_len=4, high_dim=8)
    offsets = torch.tensor([0, 2, 3, 5] if B == 3 else [0, 1], dtype=torch.int64, device=dev)
    o = {"x": torch.zeros(M, 8, device=dev), "offsets": offsets, "weight": torch.zeros(8, 8, device=dev), "logits0": None}
    return o, lambda o: capsule.capsule_ok(o["x"], o["offsets"], o["weight"], cfg, o["logits0"])


def _gate_scale(dev, B, M):
    o = {"z": torch.zeros(B, 8, device=dev), "g": torch.zeros(B, 8, device=dev), "bz": torch.zeros(8, device=dev),
         "bg": torch.zeros(8, device=dev)}
    return o, lambda o: gate_ops.gate_scale_ok([o["z"]], [o["g"]], [o["bz"]], [o["bg"]])


def _relation_chain(dev, B, M):
    o = {"x0": torch.zeros(B, 8, device=dev), "x1": torch.zeros(B, 8, device=dev), "w0": torch.zeros(8, 8, device=dev),
         "b0": torch.zeros(8, device=dev), "w1": torch.zeros(8, 16, device=dev), "b1": torch.zeros(8, device=dev)}
    return o, lambda o: gate_ops.relation_chain_ok([o["x0"], o["x1"]], [[], [0]], [[(o["w0"], o["b0"])], [(o["w1"], o["b1"])]])


def _cgc_mix(dev, B, M):
    o = {"l0": torch.zeros(B, 2, device=dev), "l1": torch.zeros(B, 2, device=dev), "e0": torch.zeros(B, 8, device=dev),
         "e1": torch.zeros(B, 8, device=dev)}
    return o, lambda o: gate_ops.cgc_mix_ok([o["l0"], o["l1"]], [o["e0"], o["e1"]], [[0, 1], [1, 0]])


def _moe_mix(dev, B, M):
    o = {"l0": torch.zeros(B, 2, device=dev), "e0": torch.zeros(B, 8, device=dev), "e1": torch.zeros(B, 8, device=dev)}
    return o, lambda o: gate_ops.moe_mix_ok([o["l0"]], [o["e0"], o["e1"]])


def _linear_rows(dev, B, M):
    o = {"x": torch.zeros(B, 16, device=dev)}
    return o, lambda o: dense.linear_rows_supported(o["x"], 16, 64)


def _linear_rows_wgrad(dev, B, M):
    o = {"g": torch.zeros(B, 64, device=dev), "x": torch.zeros(B, 16, device=dev)}
    return o, lambda o: dense.linear_rows_wgrad_supported(o["g"], o["x"], 16)


def _skinny(dev, B, M):
    o = {"x": torch.zeros(B, 8, device=dev), "weight": torch.zeros(B, 8, device=dev)}  # (B output units: the table's row count)
    return o, lambda o: dense.skinny_linear_ok(o["x"], o["weight"])


def _ln_mask(dev, B, M):
    o = {"x": torch.zeros(B, 8, device=dev), "gamma": torch.ones(8, device=dev), "beta": torch.zeros(8, device=dev)}
    return o, lambda o: masknet.ln_mask_ok(o["x"], 1, o["gamma"], o["beta"])


def _wukong(dev, B, M):
    o = {"x": torch.zeros(B, 8, device=dev), "w": torch.zeros(1, 1, device=dev)}  # (x: one feature, [B, 1, 8] when it is 2-D)
    return o, lambda o: wukong.wukong_ok(o["x"].unsqueeze(1), o["w"])


# predicate -> (its operands and call, {row operand position: the layouts it takes}, what it says about the device: "strict" = the
# device of the loaded library, "routing" = `x.is_cuda or the emulator is loaded` (a guard in front of a module's own checks),
# None = nothing, the name of its weights-like operand (sample weights, a bias, the initial logits) or None)
SPECS = {
    "match_softmax_ok": (_match, {"user": F4, "item": F4}, "strict", "weights"),
    "label_attention_ok": (_label_attention, {"item": F4}, "strict", None),
    "amm_loss_ok": (_amm, {"user_aug": F4, "item_aug": F4, "user_emb": F4, "item_emb": F4}, "strict", "weights"),
    "distill_losses_ok": (_distill, {"light": F4, "booster": F4}, "strict", "weights"),
    "capsule_ok": (_capsule, {"x": F4}, "strict", "logits0"),
    "gate_scale_ok": (_gate_scale, {"z": F4, "g": F4}, "strict", "bg"),
    "relation_chain_ok": (_relation_chain, {"x0": F4, "x1": F4}, "strict", "b1"),
    "cgc_mix_ok": (_cgc_mix, {"e0": ANY, "e1": ANY}, "strict", None),
    "moe_mix_ok": (_moe_mix, {"e0": ANY, "e1": ANY}, None, None),
    "linear_rows_supported": (_linear_rows, {"x": LEADING}, None, None),
    "linear_rows_wgrad_supported": (_linear_rows_wgrad, {"g": LEADING, "x": LEADING}, None, None),
    "skinny_linear_ok": (_skinny, {"x": ANY, "weight": SKINNY_W}, None, None),
    "ln_mask_ok": (_ln_mask, {"x": ANY}, "routing", None),
    "wukong_ok": (_wukong, {"x": ANY}, "routing", None),
}
# (the weight's shape is unpacked before anything is looked at: a 1-D weight raises, before and after)
RAISES = {("skinny_linear_ok", "weight", "one_dim")}
CASES = [(p, pos, e) for p, spec in SPECS.items() for pos in spec[1] for e in LAYOUTS + REFUSED if (p, pos, e) not in RAISES]


@pytest.mark.parametrize("pred,pos,entry", CASES, ids=["-".join(c) for c in CASES])
def test_row_operand(dev, pred, pos, entry):
    build, positions, _, _ = SPECS[pred]
    B, M = (1, 1) if entry == "one_row" else (3, 5)
    o, call = build(dev, B, M)
    assert call(o) is True
    rows, cols = o[pos].shape
    o[pos] = _entry(entry, rows, cols, dev)
    assert call(o) is (entry in positions[pos]), f"{pred}: {pos} = {entry}"


@pytest.mark.parametrize("pred", [p for p, spec in SPECS.items() if spec[2]])
def test_wrong_device_for_the_library(dev, pred):
    build, _, says, _ = SPECS[pred]
    wrong = torch.device("meta") if dev.type == "cpu" else torch.device("cpu")
    o, call = build(wrong, 3, 5)
    # (the routing guards ask only whether the emulator is loaded: its own pointer check refuses what is not host memory)
    assert call(o) is (says == "routing" and dev.type == "cpu")


@pytest.mark.parametrize("pred", [p for p, spec in SPECS.items() if spec[3]])
def test_malformed_vector(dev, pred):
    build, _, _, name = SPECS[pred]
    o, call = build(dev, 3, 5)
    shape = (5, 2) if name == "logits0" else (3,) if name == "weights" else (8,)
    o[name] = torch.zeros(shape, device=dev)
    assert call(o) is True
    wide = torch.zeros(shape[0], 2 * shape[-1], device=dev)
    for what, bad in (("a row too many", torch.zeros((shape[0] + 1,) + shape[1:], device=dev)), ("fp64", o[name].double()),
                      ("strided", wide[:, ::2] if len(shape) == 2 else wide[0, ::2][:shape[0]])):
        o[name] = bad
        assert call(o) is False, f"{pred}: {name} {what}"
    if name in ("bg", "b1"):  # a bias is read as float4 pieces: 16-byte aligned
        o[name] = torch.zeros(12, device=dev)[1:9]
        assert call(o) is False, f"{pred}: {name} misaligned"


@pytest.mark.parametrize("name,taken", [("contiguous", True), ("column_slice", True), ("misaligned", False), ("row_stride_odd", False),
                                        ("samples_apart", False), ("fp64", False)])
def test_label_attention_interests(dev, name, taken):
    """interests [B, K, D]: the B K rows of one [B K, D] row operand -- the float4 row rule with one stride between all rows"""
    o, call = _label_attention(dev, 3, 5)
    wide = torch.zeros(6, 16, device=dev)
    o["interests"] = {"contiguous": lambda: torch.zeros(3, 2, 8, device=dev), "column_slice": lambda: wide[:, 4:12].view(3, 2, 8),
                      "misaligned": lambda: wide[:, 1:9].view(3, 2, 8), "row_stride_odd": lambda: torch.zeros(6, 10, device=dev)[:, :8].view(3, 2, 8),
                      "samples_apart": lambda: torch.zeros(2, 3, 8, device=dev).transpose(0, 1),
                      "fp64": lambda: torch.zeros(3, 2, 8, device=dev).double()}[name]()
    assert o["interests"].shape == (3, 2, 8) and call(o) is taken
