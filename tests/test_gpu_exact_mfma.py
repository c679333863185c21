"""The bf16 matrix-core kernels against float64 references BIT FOR BIT, on integer operands that make every sum exact
(tests/exact_ref.py; the premise is checked on the CPU by tests/test_exact_ref_host.py over the same case lists).

The other GPU tests hold these kernels to ``rel_err <= 1e-2`` on Gaussian operands, which is right for rounding noise and
blind to one 16-row tile missing from a batch reduction, a doubled k-step, a swapped fragment slot or a wrong ReLU sign
bit.  Here every comparison is ``torch.equal(got, expect(ref, got.dtype))`` over whole tensors, and a failure names the
tensor, the number of differing elements and the first differing index.  profiles/mfma_exact_cases.md maps the case groups
to the kernel instantiations and seams they reach."""
import pytest
import torch

import exact_ref as X

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Diffs(list):
    def check(self, where, name, got, ref):
        m = X.mismatch(f"{where} {name}", got, X.expect(ref, got.dtype))
        if m:
            self.append(m)

    def zero(self, where, name, t):
        if t.numel() and float(t.float().abs().max()) != 0.0:
            self.append(f"{where} {name}: {int((t != 0).sum())} nonzero values where zeros are promised")

    def done(self):
        assert not self, "\n".join(self)


def _channels_last(x, ld):
    B, H, E = x.shape
    out = x.new_zeros(B, E, ld)
    out[:, :, :H] = x.transpose(1, 2)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cross network
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,L,rows", X.CROSS_CASES, ids=lambda v: str(v))
def test_cross_network_exact(dev, E, L, rows):
    """F_.cross_network forward and backward, both ``detach_first`` values, bf16 parameters (dW / db rounded once) and
    fp32 parameters with bf16 activations (dW / db compared without any rounding).  The cross entry has no path query:
    the shapes follow the rule in csrc/cross_mfma.hip -- cross_mfma_covers takes E in {32, 64, 96, 128} forward,
    cross_mfma_bwd E in {32, 64} with L <= 6 -- so E = 96 / 128 run the generic backward, which is held to the same
    equality (as the generic kernel would satisfy it at every other shape too)."""
    from torecsys_amd import functional as F_
    c = X.cross_case(E, L, rows)
    d = Diffs()
    gout = c.gout.to(BF16).to(dev)
    for pdt in (BF16, F32):
        for detach in (True, False):
            r = c.ref[detach]
            x = c.x.to(BF16).to(dev).requires_grad_()
            W, b = c.W.to(pdt).to(dev).requires_grad_(), c.b.to(pdt).to(dev).requires_grad_()
            out = F_.cross_network(x, W, b, detach)
            out.backward(gout)
            where = f"cross E={E} L={L} rows={rows} params={pdt} detach_first={detach}:"
            assert out.dtype == BF16 and W.grad.dtype == pdt and b.grad.dtype == pdt
            d.check(where, "out", out, r.out)
            d.check(where, "dx", x.grad, r.dx)
            d.check(where, "dW", W.grad, r.dW)
            d.check(where, "db", b.grad, r.db)
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# per-pair bilinear
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,B", X.PAIR_CASES, ids=lambda v: str(v))
def test_pair_bilinear_exact(dev, N, E, B):
    """F_._PairBilinear on the matrix-core route (_pair_mfma_fwd_ok): mode 0, mode 1 without and with the per-pair bias;
    out, gx (through the bf16 contribution rows of up to three pairs), gW (K = the batch, in sample splits), gbias"""
    from torecsys_amd import functional as F_
    c = X.pair_case(N, E, B)
    d = Diffs()
    for mode, has_bias in X.PAIR_FORMS:
        r = c.ref[(mode, has_bias)]
        x = c.x.to(BF16).to(dev).requires_grad_()
        W = c.W.to(BF16).to(dev).requires_grad_()
        bias = c.bias.to(BF16).to(dev).requires_grad_() if has_bias else None
        assert F_._pair_mfma_fwd_ok(x)
        out = F_._PairBilinear.apply(x, W, bias, mode)
        out.backward(c.gout[mode].to(BF16).to(dev))
        where = f"pair N={N} E={E} B={B} mode={mode} bias={has_bias}:"
        d.check(where, "out", out, r.out)
        d.check(where, "gx", x.grad, r.gx)
        d.check(where, "gW", W.grad, r.gW)
        if has_bias:
            d.check(where, "gbias", bias.grad, r.gbias)
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# CIN contraction, channels-last
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N,H,C,E,B,k", X.CIN_CASES, ids=lambda v: str(v))
def test_cin_contraction_exact(dev, form, N, H, C, E, B, k):
    """F_.transpose_pad + F_.cin_contract_cl: the plain form, the folded first-layer form (xkT is x0T, N > 32; the
    reference uses the unfolded weights, dx0T is the sum of both gradients), the ``live`` form of a last layer (the
    dead rows of dW exactly zero) and ``live_same``, a single unfolded layer (xkT is x0T, N <= 32) with its dead half left
    out; yT, dx0T and dxkT with their padding columns zero, dW, db; bf16 and fp32 parameters"""
    from torecsys_amd import functional as F_
    c = X.cin_case(form, N, H, C, E, B, k)
    r = c.ref
    d = Diffs()
    x0 = c.x0.to(BF16).to(dev)
    assert F_.cin_cl_supported(x0, [C], [] if H == N else [H])
    assert C in (32, 64, 128, 256)                                              # the data gradient's matrix-core set
    assert (C in (64, 128, 256) and E in (32, 64, 128)) == ((N, H, C, E) not in X.CIN_GENERIC_DW or form != "plain")
    assert F_.cin_cl_backward_route(C, E, None, 0) == (C, True, (N, H, C, E) not in X.CIN_GENERIC_DW or form != "plain")
    ld0, ldk = X.pad32(N), X.pad32(H)
    assert F_.transpose_pad_supported(x0, ld0)
    x0T_v = F_.transpose_pad(x0, ld0)
    where = f"cin {form} N={N} H={H} C={C} E={E} B={B}:"
    d.check(where, "transpose_pad", x0T_v, _channels_last(c.x0, ld0))
    gyT = c.gy.transpose(1, 2).contiguous().to(BF16).to(dev)
    for pdt in (BF16, F32):
        x0T = x0T_v.detach().clone().requires_grad_()
        xkT = x0T if c.same else _channels_last(c.xk.to(BF16), ldk).to(dev).requires_grad_()
        W, bias = c.W.to(pdt).to(dev).requires_grad_(), c.bias.to(pdt).to(dev).requires_grad_()
        yT = F_.cin_contract_cl(x0T, xkT, W, bias, N, H, live=c.live)
        yT.backward(gyT)
        w = f"{where} params={pdt}"
        d.check(w, "yT", yT, r.y.transpose(1, 2))
        d.check(w, "dx0T", x0T.grad[:, :, :N], r.dx0.transpose(1, 2))
        d.zero(w, "dx0T padding", x0T.grad[:, :, N:])
        if not c.same:
            d.check(w, "dxkT", xkT.grad[:, :, :H], r.dxk.transpose(1, 2))
            d.zero(w, "dxkT padding", xkT.grad[:, :, H:])
        assert W.grad.dtype == pdt
        d.check(w, "dW", W.grad, r.dW)
        d.check(w, "db", bias.grad, r.db)
        if c.live:
            d.zero(w, "dW dead rows", W.grad[c.live:])
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# fused MLP
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = [1, 2, 3]          # tile-in-LDS kernels, row-owner kernels, row-owner forward + tile backward


def _mlp_dev(c, dev):
    return (c.x.to(BF16).to(dev), [w.to(BF16).to(dev) for w in c.Ws], [b.to(BF16).to(dev) for b in c.bs],
            c.gout.to(BF16).to(dev))


@pytest.mark.parametrize("widths,k,rows", X.MLP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_mlp_exact(dev, widths, k, rows):
    """The raw entries and F_.fused_mlp under each kernel family request (the stacks the row-owner kernels do not cover
    resolve to the tile kernels), against the float64 reference with its OWN ReLU -- no kernel masks: integer
    pre-activations leave nothing near zero to flip.  y, the hidden activations (padding columns zero), gx, every gz and
    fp32 bias gradient of the raw backward, every dW / db through autograd."""
    from torecsys_amd import functional as F_
    c = X.mlp_case(widths, k, rows)
    r = c.ref
    widths = list(widths)
    L = len(widths) - 1
    covered = widths in X.MLP_RO_STACKS
    x, Ws, bs, gout = _mlp_dev(c, dev)
    d = Diffs()
    for req in FAMILIES:
        with F_.mlp_family(req):
            where = f"mlp {widths} rows={rows} family={req}:"
            y, hidden, masks, fam = F_.fused_mlp_forward_raw(x, Ws, bs)
            assert fam == (req if covered else F_.MLP_FAMILY_TILE)
            d.check(where, "y", y, r.y)
            for l in range(L - 1):
                d.check(where, f"hidden[{l}]", hidden[l][:, :widths[l + 1]], r.hidden[l])
                d.zero(where, f"hidden[{l}] padding", hidden[l][:, widths[l + 1]:])
            gx, gz, gb, _ = F_.fused_mlp_backward_raw(gout, widths, Ws, masks, family=fam)
            d.check(where, "gx", gx, r.gx)
            for l in range(L - 1):
                d.check(where, f"gz[{l}]", gz[l][:, :widths[l + 1]], r.gz[l])
            for l in range(L):
                d.check(where, f"gb[{l}]", gb[l][:widths[l + 1]], r.db[l])
            xd = x.clone().requires_grad_()
            Wd = [w.clone().requires_grad_() for w in Ws]
            bd = [b.clone().requires_grad_() for b in bs]
            y2 = F_.fused_mlp(xd, Wd, bd)
            y2.backward(gout)
            d.check(where, "fused_mlp y", y2, r.y)
            d.check(where, "fused_mlp dx", xd.grad, r.gx)
            for l in range(L):
                d.check(where, f"fused_mlp dW[{l}]", Wd[l].grad, r.dW[l])
                d.check(where, f"fused_mlp db[{l}]", bd[l].grad, r.db[l])
    d.done()


@pytest.mark.parametrize("widths,k,rows", X.MLP_MASK_IN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_mlp_mask_in_exact(dev, widths, k, rows):
    """mask_in form of the raw backward: the stack is fed by relu(z); gx = dL/dz (masked by the upstream ReLU) and
    gb_in its column sums, against autograd through the reference's own relu"""
    from torecsys_amd import functional as F_
    c = X.mlp_mask_in_case(widths, k, rows)
    r = c.ref
    widths = list(widths)
    covered = widths in X.MLP_RO_STACKS
    x, Ws, bs, gout = _mlp_dev(c, dev)
    d = Diffs()
    for req in FAMILIES:
        with F_.mlp_family(req):
            where = f"mlp mask_in {widths} rows={rows} family={req}:"
            y, hidden, masks, mask_in, fam = F_.fused_mlp_forward_raw(x, Ws, bs, input_mask=True)
            assert fam == (req if covered else F_.MLP_FAMILY_TILE)
            gx, gz, gb, gb_in = F_.fused_mlp_backward_raw(gout, widths, Ws, masks, mask_in, family=fam)
            d.check(where, "y", y, r.y)
            d.check(where, "gx", gx, r.gx)
            d.check(where, "gb_in", gb_in[:widths[0]], r.gb_in)
            for l in range(len(widths) - 2):
                d.check(where, f"gz[{l}]", gz[l][:, :widths[l + 1]], r.gz[l])
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# wgrad_rows, rows_gemm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f,in_f,rows", X.WGRAD_CASES, ids=lambda v: str(v))
def test_wgrad_rows_exact(dev, out_f, in_f, rows):
    """F_._wgrad_rows = g^T inp over the rows on operands kept in pad32 columns (other values behind the weight's
    columns: they must not leak in), fp32 and bf16 results, with and without the bias cast riding in the finish launch.
    From 256 rows on the matrix-core kernel is taken (trs_wgrad_rows_splits > 0, and equal to the plan restated in
    exact_ref.wgrad_splits); below, the entry's GEMM branch is held to the same equality."""
    from torecsys_amd import _abi
    from torecsys_amd import functional as F_
    c = X.wgrad_case(out_f, in_f, rows)
    g, inp = c.g.to(BF16).to(dev), c.inp.to(BF16).to(dev)
    M, N = min(g.shape[1], (out_f + 7) // 8 * 8), min(inp.shape[1], (in_f + 7) // 8 * 8)
    S = int(_abi.load().trs_wgrad_rows_splits(M, N, rows))
    assert S == X.wgrad_splits(M, N, rows) and (S > 0) == (rows >= 4 * X.WG_KR)
    gb_f32 = torch.zeros(X.pad32(out_f), dtype=F32, device=dev)
    gb_f32[:out_f] = c.db.to(F32).to(dev)
    d = Diffs()
    for dtype in (F32, BF16):
        where = f"wgrad_rows {out_f}x{in_f} rows={rows} S={S} {dtype}:"
        d.check(where, "dW", F_._wgrad_rows(g, inp, out_f, in_f, dtype), c.dW)
        dW, db = F_._wgrad_rows(g, inp, out_f, in_f, dtype, gb_f32)
        assert dW.dtype == dtype and db.dtype == dtype
        d.check(where, "dW (with gb_f32)", dW, c.dW)
        d.check(where, "db", db, c.db)
    d.done()


@pytest.mark.parametrize("out_f,in_f,rows,k", X.ROWS_GEMM_CASES, ids=lambda v: str(v))
def test_rows_gemm_exact(dev, out_f, in_f, rows, k):
    """F_.rows_gemm: y = g[:, :out_f] @ W[:out_f] on the matrix cores (rows_gemm_supported), rows one into the second pass
    of the persistent loop and ragged last tiles, other values in g's columns behind the zero padding"""
    from torecsys_amd import functional as F_
    c = X.rows_gemm_case(out_f, in_f, rows, k)
    x, W = c.x.to(BF16).to(dev), c.W.to(BF16).to(dev)
    assert F_.rows_gemm_supported(x, W, out_f, in_f)
    y = F_.rows_gemm(x, W, out_f, in_f)
    d = Diffs()
    d.check(f"rows_gemm {out_f}x{in_f} rows={rows}:", "y", y, c.y)
    d.done()
