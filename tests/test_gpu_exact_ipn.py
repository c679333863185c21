"""Every inner-product (IPN) kernel path of csrc/pair.hip against the float64 reference BIT FOR BIT, on integer operands
that make every sum exact in bf16 and fp32 alike (tests/exact_ipn_ref.py; the premise, the restated dispatch arithmetic and
the thresholds the case lists sit on are checked on the CPU by tests/test_exact_ipn_host.py over the same lists).

The tolerance tests hold these kernels to 1e-2 at a handful of shapes, none on a 16-field tile edge, none with four field
tiles at E = 64 / 128, one above the 8192 samples from which a wave takes a second sample.  Here every comparison is
``torch.equal(got, expect(ref, got.dtype))`` over whole tensors; a failure names the tensor, the number of differing
elements and the first differing index.  profiles/mfma_exact_cases.md maps the case groups to the kernels and seams."""
import os
import subprocess
import sys

import pytest
import torch

import exact_ipn_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = R.BF16, R.F32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _pair_dot(dev, dtype, c, where, x=None):
    """forward and backward of F_.pair_dot on the case's operands (``x``: a device tensor to use instead of a fresh one)"""
    from torecsys_amd import functional as F_
    d = Diffs()
    if x is None:
        x = c.x.to(dtype).to(dev)
    x.requires_grad_()
    out = F_.pair_dot(x)
    (dx,) = torch.autograd.grad(out, x, c.gout.to(dtype).to(dev))
    assert out.dtype == dtype and dx.dtype == dtype
    d.check(where, "out", out, c.out)
    d.check(where, "dx", dx, c.dx)
    d.done()


@pytest.mark.parametrize("N,E,B", R.IPN_MFMA_N, ids=str)
def test_ipn_mfma_field_tiles_exact(dev, N, E, B):
    """bf16 matrix-core kernels, every NT x KS (forward) / NT x KE (backward), N on both sides of every 16-field tile edge:
    the ``i < j && j < N`` store filter, the ``row < N`` load filter, the zero padding of Gs / X^T"""
    p = R.ipn_path(BF16, N, E)
    _pair_dot(dev, BF16, R.ipn_case(N, E, B), f"ipn mfma<{p.NT},{p.KS}|{p.KE}> N={N} E={E} B={B}:")


@pytest.mark.parametrize("N,E,B", R.IPN_MFMA_B, ids=str)
def test_ipn_mfma_samples_per_wave_exact(dev, N, E, B):
    """the grid cap of 2048 blocks: up to 8192 samples one per wave, 8193 a second for wave 0, 16385 a third -- the
    backward's prefetch chain hands over a different next sample once / twice and clamps on the last"""
    _pair_dot(dev, BF16, R.ipn_case(N, E, B), f"ipn mfma N={N} E={E} B={B}:")


@pytest.mark.parametrize("dtype,N,E", R.IPN_SLOT, ids=R.dtype_tag)
def test_ipn_slot_map_exact(dev, dtype, N, E):
    """one sample per pair with two live fields and a one-hot gradient: forward E * I_P, backward +-v_p on fields i_p and
    j_p only -- pair_index and the backward's lut, pair by pair, in every kernel family"""
    p = R.ipn_path(dtype, N, E)
    _pair_dot(dev, dtype, R.slot_case(N, E), f"ipn slots {p.fwd}/{p.bwd} {R.dtype_tag(dtype)} N={N} E={E}:")


@pytest.mark.parametrize("dtype,N,E,B", R.IPN_TILE + R.IPN_BUDGET + R.IPN_GENERIC, ids=R.dtype_tag)
def test_ipn_tile_and_generic_exact(dev, dtype, N, E, B):
    """the LDS-tile kernels (4 x 4 register tiles; N mod 4, a second tile per lane from N = 41 on), the hand-over to the
    generic kernels at the LDS budget separately per direction, and the generic kernels proper (E % 4 != 0, N = 65)"""
    p = R.ipn_path(dtype, N, E)
    _pair_dot(dev, dtype, R.ipn_case(N, E, B), f"ipn {p.fwd}/{p.bwd} {R.dtype_tag(dtype)} N={N} E={E} B={B}:")


def test_ipn_unaligned_view_exact(dev):
    """a contiguous bf16 block that starts one element into its buffer: inside the matrix-core set, but its rows are not
    16-byte aligned -- both entries hand it to the tile kernels, which stage it with scalar loads"""
    N, E, B = R.UNALIGNED_CASE
    c = R.ipn_case(N, E, B)
    buf = torch.zeros(B * N * E + 8, dtype=BF16, device=dev)
    x = buf[1:1 + B * N * E].view(B, N, E)
    x.copy_(c.x.to(BF16))
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    _pair_dot(dev, BF16, c, f"ipn unaligned N={N} E={E} B={B}:", x=x)


@pytest.mark.parametrize("N,E,B,it", R.IPN_EMBED, ids=R.dtype_tag)
def test_embed_ipn_exact(dev, N, E, B, it):
    """F_.embed_ipn (the gather-fused forward + the matrix-core backward + the row scatter): the block, the products and
    the table gradient with BOTH output gradients flowing; the inference form without the block; one id out of range:
    a zero row, no gradient, the index flag raised"""
    from torecsys_amd import functional as F_
    c = R.embed_case(N, E, B, it)
    d = Diffs()
    where = f"embed_ipn N={N} E={E} B={B} {R.dtype_tag(it)}:"
    off, ge, gp = c.offsets.to(dev), c.ge.to(BF16).to(dev), c.gp.to(BF16).to(dev)
    F_.index_errors_seen()                                                  # clear what earlier tests left
    for name, ids, r in (("", c.idx, c.ref), (" (one id out of range)", c.bad, c.oob)):
        w = c.table.to(BF16).to(dev).requires_grad_()
        assert F_.embed_ipn_supported(w, N)
        idx = ids.to(dev)
        emb, ipn = F_.embed_ipn(w, idx, off)
        (gw,) = torch.autograd.grad([emb, ipn], w, [ge, gp])
        d.check(where + name, "emb", emb, r.emb)
        d.check(where + name, "ipn", ipn, r.out)
        d.check(where + name, "table gradient", gw, r.gtab)
        with torch.no_grad():
            none, ipn2 = F_.embed_ipn(w.detach(), idx, off, want_emb=False)
        assert none is None
        d.check(where + name, "ipn without the block", ipn2, r.out)
        assert F_.index_errors_seen() == (ids is c.bad), where + name
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# the backward's dynamic LDS inside one (NT, KE) instantiation
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys, torch
import exact_ipn_ref as R
from torecsys_amd import functional as F_
dev = torch.device("cuda:0")
bad = 0
for E, Ns in R.IPN_LDS_BUCKETS:
    state = "OK"
    for N in Ns:
        c = R.ipn_case(N, E, 5)
        x = c.x.to(R.BF16).to(dev).requires_grad_()
        out = F_.pair_dot(x)
        try:
            (dx,) = torch.autograd.grad(out, x, c.gout.to(R.BF16).to(dev))
            torch.cuda.synchronize()
        except RuntimeError as e:
            msg = str(e)
            state = f"LAUNCH-FAILED at N={N} lds={R.bwd_mfma_lds(N, E)}: {msg[:300]}"
            if "pair_dot_bwd" not in msg:          # anything but the launch's own API error: stop here
                print(f"BUCKET E={E} N={Ns}: {state}", flush=True)
                sys.exit(3)
            break
        m = R.mismatch(f"dx N={N} E={E}", dx, R.expect(c.dx, R.BF16)) or R.mismatch(f"out N={N} E={E}", out, R.expect(c.out, R.BF16))
        if m:
            state = "MISMATCH " + m
            break
    bad += state != "OK"
    print(f"BUCKET E={E} N={Ns}: {state}", flush=True)
print("IPN-LDS-BUCKETS OK" if not bad else f"IPN-LDS-BUCKETS {bad} BAD")
"""


def test_backward_lds_grows_within_a_tile_bucket():
    """pair_dot_bwd_mfma asks for ((P + 7) & ~7) * 2 bytes of pair table on top of its per-wave images, so its dynamic LDS
    grows with N INSIDE one <NT, KE> instantiation, above 64 KiB from N = 33 on -- and the function attribute that admits
    more than 64 KiB is per instantiation and per process.  A fresh process (other tests may have raised the attribute
    already) runs each instantiation's backward in ascending order of N, every result compared exactly."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "IPN-LDS-BUCKETS OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count(": OK") == len(R.IPN_LDS_BUCKETS)
