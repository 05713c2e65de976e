"""tests/bf3_ref.py pinned, and the proof -- before any GPU is involved -- that tests/test_gpu_bf3_terms.py can tell the six-term
contract from an arithmetic that lost one of its third-order products.  No GPU, no library."""
import numpy as np
import pytest
import torch

import bf3_ref as R


def _bits(x):
    return x.contiguous().view(torch.int32)


def _split_inputs():
    g = torch.Generator().manual_seed(1)
    yield "randn", torch.randn(1 << 16, generator=g)
    # 1e-30 .. 1e30, both signs (the lo term of 1e-30 is still a normal number)
    mag = 10.0 ** (60.0 * torch.rand(1 << 16, generator=g, dtype=torch.float64) - 30.0)
    yield "1e-30..1e30", (mag * torch.randn(1 << 16, generator=g, dtype=torch.float64).sign()).float()
    # few mantissa bits: the residues are short or zero
    m = torch.randint(1, 16, (1 << 12,), generator=g).float() * 2.0 ** torch.randint(-20, 20, (1 << 12,), generator=g).float()
    yield "few bits", torch.cat([m, -m, torch.zeros(4), torch.tensor([1.0, -1.0, 0.5, 3.0])])
    # every mantissa bit set, and a lone last bit below a run of zeros
    yield "edges", torch.tensor([1.9999999, 1.0000001, -1.9999999, 255.99998, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -16 + 2.0 ** -23])


@pytest.mark.parametrize("what,x", list(_split_inputs()), ids=lambda v: v if isinstance(v, str) else "")
def test_split3_is_exact_and_truncating(what, x):
    hi, mid, lo = R.split3(x)
    # bit for bit, summed in fp32 in the order the terms were taken off ...
    assert torch.equal(_bits((lo + mid) + hi), _bits(x)), what
    # ... and as real numbers
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double()), what
    for t in (hi, mid, lo):                                       # every term is a bf16 number
        assert torch.all((_bits(t) & 0xFFFF) == 0), what
    # truncation, not rounding: a term never exceeds what it was taken from, and has its sign
    assert torch.all(hi.abs() <= x.abs()) and torch.all(hi * x >= 0), what
    r1 = x - hi
    assert torch.all(mid.abs() <= r1.abs()) and torch.all(mid * r1 >= 0), what
    # the kernels' own words for it (pack_device.h): the top 16 bits
    u = x.numpy().view(np.uint32)
    assert np.array_equal(hi.numpy().view(np.uint32), u & np.uint32(0xFFFF0000)), what


@pytest.mark.parametrize("K", [8, 136, 648])
def test_contract_is_close_to_the_true_product_sum(K):
    """The three dropped products (mid*lo, lo*mid, lo*lo) are all that separates the contract from the exact sum: within
    3 * 2^-24 of sum |a| |b|, element by element.  (A truncated mid term is below 2^-7 and a lo term below 2^-15 of its value, so
    one adversarial product can reach 2^-21; on inputs of the suite's kind the terms' means are a quarter of that.)"""
    g = torch.Generator().manual_seed(K)
    a = torch.randn(64, K, generator=g) * K ** -0.5
    b = torch.randn(K, 256, generator=g)
    em, ct = R.six_term(a, b)
    true = a.double() @ b.double()
    room = a.double().abs() @ b.double().abs()
    assert torch.all((ct - true).abs() <= 3 * 2.0 ** -24 * room)
    # the emulation rounds into fp32 three times per chunk: it stays an fp32 computation of the same sum
    assert torch.all((em.double() - ct).abs() <= 3 * (K // 8) * 2.0 ** -24 * room)


def test_missing_removes_exactly_one_product_over_the_channels_named():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(16, 24, generator=g), torch.randn(24, 32, generator=g)
    ta, tb = [t.double() for t in R.split3(a)], [t.double() for t in R.split3(b)]
    _, ct = R.six_term(a, b)
    for name, (i, j) in R.THIRD_ORDER.items():
        _, m = R.six_term(a, b, missing=(name, slice(8, 16)))
        assert torch.equal(ct - m, ta[i][:, 8:16] @ tb[j][8:16]), name
        _, m = R.six_term(a, b, missing=(name, slice(None)))
        assert torch.allclose(ct - m, ta[i] @ tb[j], rtol=0, atol=1e-15), name


def test_adapters_compute_the_convolution_and_the_attention():
    """each adapter's contract against the float64 torch op: the operands are where the kernel puts them"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g)
    x, x2 = r(2, 10, 9, 7), r(2, 6, 9, 7)
    w3, w1, b = r(5, 16, 3, 3) * 0.1, r(5, 16, 1, 1) * 0.25, r(5)
    gn = (1.0 + 0.3 * r(2, 16), 0.3 * r(2, 16))
    xx = torch.cat([x, x2], 1)
    pro = F.silu(xx.double() * gn[0].double()[:, :, None, None] + gn[1].double()[:, :, None, None])
    tol = dict(rtol=0, atol=2e-6)
    ref = F.conv2d(pro, w3.double(), b.double(), padding=1)
    assert torch.allclose(R.winograd_3x3(x, w3, b, gn, True, x2)[1], ref, **tol)
    ref = F.conv2d(F.interpolate(xx.double(), scale_factor=2.0, mode="nearest"), w3.double(), b.double(), padding=1)
    assert torch.allclose(R.winograd_3x3(xx, w3, b, upsample=True)[1], ref, **tol)
    assert torch.allclose(R.direct_1x1(xx, w1, b)[1], F.conv2d(xx.double(), w1.double(), b.double()), **tol)
    ref = F.conv2d(xx.double(), w3.double(), b.double(), stride=2, padding=1)
    assert torch.allclose(R.direct_3x3_s2(xx, w3, b)[1], ref, **tol)
    # a mutant over some channels of the unfolded form is the same mutant of the convolution restricted to them
    m = R.direct_3x3_s2(xx, w3, b, missing=("hi*lo", slice(8, 16)))[1]
    m8 = R.direct_3x3_s2(xx[:, 8:16].contiguous(), w3[:, 8:16].contiguous(), None, missing=("hi*lo", slice(None)))
    c8 = R.direct_3x3_s2(xx[:, 8:16].contiguous(), w3[:, 8:16].contiguous(), None)[1]
    assert torch.allclose(R.direct_3x3_s2(xx, w3, b)[1] - m, c8 - m8[1], rtol=0, atol=1e-12)
    qkv = r(2, 3 * 16, 37) * 1.5
    q, k, v = qkv.double().reshape(2, 3, 2, 8, 37).unbind(1)
    p = torch.softmax(torch.einsum("bhdq,bhdk->bhqk", q, k) * 8 ** -0.5, dim=-1)
    ref = torch.einsum("bhqk,bhdk->bhdq", p, v).reshape(2, 16, 37)
    assert torch.allclose(R.attention(qkv, 2)[1], ref, **tol)


def test_one_active_chunk_is_the_same_run_contracted_over_that_chunk():
    """reference() contracts a one-chunk run over its eight active channels only: the full contraction gives the same bits"""
    case = next(c for c in R.CASES if c.kind == "wino" and c.c1)              # the concatenated one, seam inside chunk 2
    for chunk in (0, 2, 4):
        t = R.inputs(case, chunk)
        full = R.winograd_3x3(t["x"], t["w"], t["bias"], t["gn"], True, t["x2"])
        ref = R.reference(case, chunk)
        assert torch.equal(full[1], ref.contract)
        x = torch.cat([t["x"], t["x2"]], 1)
        off = torch.ones(case.cin, dtype=torch.bool)
        off[8 * chunk:8 * chunk + 8] = False
        assert not x[:, off].any() and not t["gn"][0][:, off].any() and not t["gn"][1][:, off].any()
        assert x[:, ~off].abs().min() > 0


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.ident)
def test_every_gpu_case_separates_the_contract_from_its_mutants(case):
    """d_mut >= 16 * d_emul for every run of every case of tests/test_gpu_bf3_terms.py (the same table): the GPU bound
    d_mut / 4 leaves a correct kernel four times the emulation's own distance and stays four times under the least visible
    mutant."""
    worst = None
    for chunk in R.runs(case):
        ref = R.reference(case, chunk)
        ratio = ref.d_mut / ref.d_emul
        if worst is None or ratio < worst[0]:
            worst = (ratio, chunk, ref.d_emul, ref.d_mut)
        assert ref.d_mut >= R.SEPARATION * ref.d_emul, \
            f"{case.ident} chunk {chunk}: d_mut {ref.d_mut:.3e} < 16 * d_emul {ref.d_emul:.3e} ({ref.mutants})"
    print(f"{case.ident}: least separation {worst[0]:.1f} at chunk {worst[1]} (d_emul {worst[2]:.2e}, d_mut {worst[3]:.2e})")


@pytest.mark.parametrize("K", [136, 648])
def test_the_parity_bound_cannot_see_a_one_chunk_mutant(K):
    """Why this file exists, as a checked fact: on dense inputs of the suite's kind (randn inputs, weights scaled by K**-0.5) an
    arithmetic that loses a third-order product in ONE 8-channel chunk lies inside the parity tests' 1e-5 * max(1, |ref|)
    of the float64 convolution -- every product, every chunk tried.  (With only that chunk active the same mutant is 1e-5 of
    the largest output away, the separation test above.)"""
    g = torch.Generator().manual_seed(K)
    x = torch.randn(2, K, 16, 16, generator=g)
    w = torch.randn(128, K, 1, 1, generator=g) * K ** -0.5
    ref64 = torch.nn.functional.conv2d(x.double(), w.double())
    bound = 1e-5 * max(1.0, ref64.abs().max().item())
    for chunk in (0, K // 16, K // 8 - 1):
        for prod in R.THIRD_ORDER:
            em, _ = R.direct_1x1(x, w, missing=(prod, slice(8 * chunk, 8 * chunk + 8)))
            assert (em - ref64).abs().max().item() < bound, f"{prod} chunk {chunk}: the old bound sees it after all"
