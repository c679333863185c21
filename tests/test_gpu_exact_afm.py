"""Every attentional-FM kernel path of csrc/afm.hip against the float64 reference BIT FOR BIT, on operands that make the
softmax and everything behind it exact in bf16 and fp32 alike (tests/exact_afm_ref.py; the premise, the coverage conditions,
the restated dispatch arithmetic and the thresholds the case lists sit on are checked on the CPU by
tests/test_exact_afm_host.py over the same lists).

The tolerance tests hold these kernels to 1e-2 at 14 shapes, none above N = 39, one with a second sample per workgroup of
the matrix-core backward (at N = 2), none above the other grid caps.  Here every comparison is
``torch.equal(got, expect(ref, got.dtype))`` over whole tensors -- ``F_.afm`` forward plus backward: out, attn, gx and all
four parameter gradients; a failure names the tensor, the number of differing elements and the first differing index.
profiles/mfma_exact_cases.md maps the case groups to the kernels and seams."""
import pytest
import torch

import exact_afm_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = R.BF16, R.F32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Diffs(list):
    def check(self, where, name, got, ref):
        m = R.mismatch(f"{where} {name}", got, R.expect(ref, got.dtype))
        if m:
            self.append(m)

    def done(self):
        assert not self, "\n".join(self)


def _afm(dev, dtype, c, where, x=None, backward=True):
    """forward and backward of F_.afm on the case's operands (``x``: a device tensor to use instead of a fresh one);
    ``backward`` False: the entry refuses the shape's backward (more than 160 KiB of LDS) and has to say so"""
    from torecsys_amd import functional as F_
    d = Diffs()
    r = c.ref
    put = lambda t: None if t is None else t.to(dtype).to(dev)             # noqa: E731
    if x is None:
        x = put(c.x)
    x.requires_grad_()
    ps = [put(c.W1).requires_grad_(), put(c.b1).requires_grad_(), put(c.w2).view(1, -1).requires_grad_(), put(c.b2).requires_grad_()]
    keep = None if c.keep is None else c.keep.to(dev)
    out, attn = F_.afm(x, *ps, keep, c.keep_scale)
    assert out.dtype == dtype and attn.dtype == dtype
    d.check(where, "out", out, r.out)
    d.check(where, "attn", attn, r.attn)
    heads = [(out, c.g_out), (attn, c.g_attn)]
    outs, gs = [h for h, g in heads if g is not None], [put(g) for h, g in heads if g is not None]
    if not backward:
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            torch.autograd.grad(outs, [x] + ps, gs)
        d.done()
        return
    gx, gW1, gb1, gw2, gb2 = torch.autograd.grad(outs, [x] + ps, gs)
    torch.cuda.synchronize()
    assert gx.dtype == dtype and gW1.dtype == dtype
    d.check(where, "gx", gx, r.gx)
    d.check(where, "gW1", gW1, r.gW1)
    d.check(where, "gb1", gb1, r.gb1)
    d.check(where, "gw2", gw2.view(-1), r.gw2)
    d.check(where, "gb2", gb2, r.gb2)
    d.done()


def _where(case):
    dt, N, E, A = case[:4]
    p = R.afm_path(N, E, A, dt)
    fwd = f"fwd_mfma<{p.fwd_AT},{E // 32}>" if p.fwd == "mfma" else "fwd generic"
    bwd = (f"bwd_mfma<{p.bwd_AT},{E // 32}> {p.sched}" if p.bwd == "mfma" else
           f"bwd generic<{p.AMAX},{p.ES}>" if p.bwd == "generic" else "bwd refused")
    return f"afm {R.case_id(case)} [{fwd} | {bwd}]:", p


def _case(dev, case):
    where, p = _where(case)
    _afm(dev, case[0], R.afm_case(*case), where, backward=p.bwd != "unsupported")


@pytest.mark.parametrize("case", R.AFM_INST, ids=R.case_id)
def test_afm_instantiations_exact(dev, case):
    """bf16, every forward <A / 16, E / 32>; the backward on the matrix cores where A % 32 == 0 and AT KS <= 12, on the
    generic kernels elsewhere (the hand-over between the families inside one autograd op); at (112, 128) and (128, 128)
    the entry refuses the backward -- the generic kernel's LDS is asked of every shape -- and says so"""
    _case(dev, case)


@pytest.mark.parametrize("case", R.AFM_SCHED, ids=R.case_id)
def test_afm_backward_tile_schedules_exact(dev, case):
    """the three tile schedules of the matrix-core backward: fewer tiles than waves (N = 2..4), the rounds as they are, the
    host-packed tiles up to N = 60, TPR = 2 (N = 61, 64) and TPR = 3 (N = 65, past the packer's 64-bit field mask); waves
    that end a sample on an odd tile count feed GEMM (3) a zero-filled second half"""
    _case(dev, case)


@pytest.mark.parametrize("dtype,N,E,A", R.AFM_SLOT, ids=R.dtype_tag)
def test_afm_slot_map_exact(dev, dtype, N, E, A):
    """one sample per pair, live on that pair only: attn is the identity, out[p] the product row of pair p, gx touches
    fields i_p and j_p alone -- pair_ij, the forward's lut, the backward's lutp and every schedule slot, pair by pair"""
    where, _ = _where((dtype, N, E, A, N * (N - 1) // 2, "slot"))
    _afm(dev, dtype, R.slot_case(N, E, A), where)


@pytest.mark.parametrize("case", R.AFM_CAP_BWD + R.AFM_CAP_FWD + R.AFM_CAP_GENERIC, ids=R.case_id)
def test_afm_grid_caps_exact(dev, case):
    """matrix-core backward: 256 workgroups, B = 256 / 257 / 513 give workgroup 0 one / two / three samples, at N = 17 and
    N = 39 where a wave ends every sample on an odd tile count (the next sample starts again at column 0 of the 32-pair
    step, its private gradient block zeroed, dW1 carried on in registers); matrix-core forward: 2049
    samples are more than any resident grid; generic kernels: 1024 workgroups, B = 1024 / 1025 in both dtypes"""
    _case(dev, case)


@pytest.mark.parametrize("case", R.AFM_GENERIC, ids=R.case_id)
def test_afm_generic_kernels_exact(dev, case):
    """afm_fwd_kernel<T> / afm_bwd_kernel<T, AMAX, ES> in fp32 and bf16: every AMAX x ES with A on the bucket edges, E and A
    that are no multiple of 4, and more than 64 KiB of LDS in both directions (the attribute branch)"""
    _case(dev, case)


def test_afm_unaligned_view_exact(dev):
    """a contiguous bf16 block that starts one element into its buffer: inside the matrix-core set of both directions, but
    not 16-byte aligned -- both entries hand it to the generic kernels.  The Python entry passes the view through uncopied
    (``contiguous()`` of a contiguous view is the view)."""
    case = R.UNALIGNED_CASE
    dt, N, E, A, B = case[:5]
    c = R.afm_case(*case)
    buf = torch.zeros(B * N * E + 8, dtype=BF16, device=dev)
    x = buf[1:1 + B * N * E].view(B, N, E)
    x.copy_(c.x.to(BF16))
    assert x.is_contiguous() and x.data_ptr() % 16 != 0 and x.contiguous().data_ptr() == x.data_ptr()
    p = R.afm_path(N, E, A, dt, aligned=False)
    assert p.fwd == p.bwd == "generic"
    _afm(dev, dt, c, f"afm unaligned {R.case_id(case)}:", x=x)


@pytest.mark.parametrize("case", R.AFM_DROP + R.AFM_MODES, ids=R.case_id)
def test_afm_score_dropout_and_absent_gradients_exact(dev, case):
    """keep_scale 2 and 4 with a fixed mask (dropped scores exactly 0, the sum and the backward see the dropped scores), and
    one of the two output gradients absent (None reaches the kernel as a null pointer), on both families"""
    _case(dev, case)
