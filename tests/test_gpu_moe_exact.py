"""The three kernels of csrc/moe.hip against a float64 softmax BIT FOR BIT: every (lane-group width, vectors per lane)
instantiation of moe_gate_group_kernel in both dtypes with a full and a partly filled last round, the element kernels at
row lengths round the wave and the backward's 512-column tile, unaligned operands, and second trips of all three
grid-stride loops (tests/gate_exact_ref.py: rows whose live columns share one integer logit and whose dead columns sit at
-20000, so P is 1 / n or 0 with n a power of two; tests/test_gate_exact_host.py proves that exact and the lists complete).

Premise: the device gives expf(0) == 1 and expf(-20000) == 0 (tests/exact_attn_ref.py rests on the first as well).  Every
comparison is ``torch.equal`` with the float64 value rounded once; a failure names the tensor, the number of differing
elements and the first differing index.  Each case asserts the branch the library reports against the rule written out in
``_path_rule``.  profiles/gate_exact_cases.md maps the cases to the instantiations."""
import pytest
import torch

import gate_exact_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = R.F32, R.BF16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _path_rule(K, dtype, aligned=True):
    """vector path: rows of whole 16-byte vectors (and whole quads of fp32 logits), at most 64 lanes x 16 columns, every
    pointer on a 16-byte boundary"""
    size = 4 if dtype == F32 else 2
    return 1 if (K % 4 == 0 and (K * size) % 16 == 0 and K <= 1024 and aligned) else 2


def _off(t):
    """the same values one element off a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 in (2, 4)
    return v


def _run(dev, dtype, o, where, d, off=None):
    from torecsys_amd import functional as F_
    assert (F_.MOE_PATH_VECTOR, F_.MOE_PATH_ELEMENT) == (R.VECTOR, R.ELEMENT) == (1, 2)
    r = R.moe_ref(o)
    ops = [o.logits.to(F32).to(dev), None if o.bias is None else o.bias.to(dtype).to(dev), o.experts.to(dtype).to(dev),
           o.gout.to(dtype).to(dev)]
    if off is not None:
        ops[off] = _off(ops[off])
    fwd_aligned = off is None or off == 3                                        # gout: the backward's operand only
    fwd_path, bwd_path = _path_rule(o.K, dtype, fwd_aligned), _path_rule(o.K, dtype, off is None)
    assert (fwd_path, bwd_path) == (R.moe_path(o.K, dtype, fwd_aligned), R.moe_path(o.K, dtype, off is None))
    out = F_.moe_gate_forward_raw(*ops[:3])
    assert F_.moe_gate_last_path() == fwd_path, (where, "forward")
    gl, ge = F_.moe_gate_backward_raw(*ops)
    assert F_.moe_gate_last_path() == bwd_path, (where, "backward")
    assert out.dtype == gl.dtype == ge.dtype == dtype
    d.check(where, "out", out, r.out)
    d.check(where, "glogits", gl, r.glogits.view(o.B, o.G * o.K))
    d.check(where, "gexperts", ge, r.gexperts)


def _run_all_forms(dev, dtype, K, what):
    d = R.Diffs()
    for G in R.MOE_GS:
        for bias in (False, True):
            o = R.moe_operands(R.MOE_B, G, K, bias)
            _run(dev, dtype, o, f"moe {what} {R.dt_tag(dtype)} K{K} G{G} {'bias' if bias else 'no bias'}:", d)
    torch.cuda.synchronize()
    d.done()


def test_the_device_exponential_is_exact_where_the_operands_need_it(dev):
    """the premise: one live column beside one dead one gives P = (1, 0) exactly, through either path"""
    from torecsys_amd import functional as F_
    for K in (4, 2):
        logits = torch.full((1, K), R.MOE_DEAD, device=dev)
        logits[0, 0] = 3.0
        out = F_.moe_gate_forward_raw(logits, None, torch.ones(1, K, device=dev))
        assert out.view(-1).tolist() == [1.0] + [0.0] * (K - 1), "expf(0) != 1 or expf(-20003) != 0 on this device"
        out = F_.moe_gate_forward_raw(torch.full((1, K), 3.0, device=dev), None, torch.ones(1, K, device=dev))
        assert out.view(-1).tolist() == [1.0 / K] * K


@pytest.mark.parametrize("case", R.MOE_VECTOR_CASES, ids=R.moe_case_id)
def test_vector_path_every_group_width_exact(dev, case):
    """lg 0 .. 5 with one vector per lane, lg 6 with 1, 2 and (fp32) 3 or 4; K a whole number of rounds and K one vector
    past it, where the last lanes of a group own nothing and feed -inf / 0 to the group's maximum and sums"""
    dtype, K = case
    assert _path_rule(K, dtype) == 1
    _run_all_forms(dev, dtype, K, "lg %d R %d %s" % (R.moe_group(K, dtype)[:2] + (R.moe_fill(K, dtype),)))


@pytest.mark.parametrize("case", R.MOE_ELEMENT_CASES, ids=R.moe_case_id)
def test_element_path_exact(dev, case):
    """rows shorter than, equal to and past a wave's 64 lanes and the backward's 512-column tile; K = 1028 has a vector
    shape above the cap; bf16 rows of 4, 12, 20 columns are multiples of 4 and no whole vectors"""
    dtype, K = case
    assert _path_rule(K, dtype) == 2
    _run_all_forms(dev, dtype, K, "element, %d tile(s)" % R.moe_bwd_tiles(K))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dt_tag)
def test_unaligned_operands_take_the_element_path_exact(dev, dtype):
    """a vector shape with logits, bias, experts or gout 4 or 2 bytes off a 16-byte boundary"""
    K = R.MOE_UNALIGNED_K
    d = R.Diffs()
    o = R.moe_operands(R.MOE_B, 3, K, True)
    for which, name in enumerate(("logits", "bias", "experts", "gout")):
        _run(dev, dtype, o, f"moe {R.dt_tag(dtype)} K{K}, {name} off the boundary:", d, off=which)
    torch.cuda.synchronize()
    d.done()


@pytest.mark.parametrize("case", R.MOE_TRIP_VECTOR, ids=R.moe_case_id)
def test_vector_path_second_trip_exact(dev, case):
    """more lane groups than 4096 workgroups of 256 lanes hold: the first groups take a second sample"""
    dtype, K, G, B = case
    lg = R.moe_group(K, dtype)[0]
    assert B << lg > 4096 * 256 and _path_rule(K, dtype) == 1
    d = R.Diffs()
    _run(dev, dtype, R.moe_operands(B, G, K, True), f"moe second trip {R.moe_case_id(case)}:", d)
    torch.cuda.synchronize()
    d.done()


@pytest.mark.parametrize("case", R.MOE_TRIP_ELEMENT, ids=R.moe_case_id)
def test_element_path_second_trip_exact(dev, case):
    """more rows (forward) and samples (backward) than the 16 384 waves of the grid"""
    dtype, K, G, B = case
    assert B * G * 64 > 4096 * 256 and B * 64 > 4096 * 256 and _path_rule(K, dtype) == 2
    d = R.Diffs()
    _run(dev, dtype, R.moe_operands(B, G, K, True), f"moe second trip {R.moe_case_id(case)}:", d)
    torch.cuda.synchronize()
    d.done()
