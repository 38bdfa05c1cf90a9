"""tests/lora_rows_ref.py before anything is tied to it: each float64 restatement against a plain triple loop, the mask layout against
oracle.philox, the fp32 stand-in inside a sanity rail on every case, the exact cases exact (reference == stand-in bit for bit, bf16 results
unrounded), every mutant outside what a device is allowed on every listed case it applies to, the case lists reaching every cut of the four
kernels, and every masked tn case drawing a mask that makes each quad exchange matter.  No GPU."""
import pytest
import torch

import gemm_ref
import lora_rows_ref as R
from oracle import philox

F64 = torch.float64
IDS = [c.name for c in R.CASES]
EXACT_IDS = [c.name for c in R.EXACT_CASES]


def test_the_constants_are_gemm_refs():
    assert R.FACTOR is gemm_ref.FACTOR and R.FLOOR is gemm_ref.FLOOR and (R.FACTOR, R.FLOOR) == (8.0, 2.0 ** -22)


@pytest.mark.parametrize('M,K,N,r', [(16, 32, 32, 3), (32, 64, 32, 16)])
def test_references_equal_a_plain_triple_loop(M, K, N, r):
    g = torch.Generator().manual_seed(M + K)
    bf = lambda *s: torch.randn(*s, generator=g).bfloat16()
    drop = R.Drop(0.25, 5, 2, 1)
    scale = 0.75
    ks = 1.0 / 0.75
    x, P, u, B, y0 = bf(M, K), bf(R.RP, K), bf(M, R.RP), bf(N, R.RP), bf(M, N)
    flat = philox.dropout_mask(M * max(K, N), 0.25, 5, 2, 1)
    kx = [[float(philox.dropout_mask(M * K, 0.25, 5, 2, 1)[i * K + k] != 0) for k in range(K)] for i in range(M)]
    my = [[float(philox.dropout_mask(M * N, 0.25, 5, 2, 1)[i * N + n]) for n in range(N)] for i in range(M)]
    assert 0 < (flat == 0).mean() < 1
    xl, Pl, ul, Bl, yl = (t.double().tolist() for t in (x, P, u, B, y0))

    down = [[scale * ks * sum(kx[i][k] * xl[i][k] * Pl[j][k] for k in range(K)) for j in range(R.RP)] for i in range(M)]
    got = R.down64(x, P, scale, drop)
    assert torch.allclose(got, torch.tensor(down, dtype=F64), rtol=1e-13, atol=1e-14)

    up = [[yl[i][n] + scale * my[i][n] * sum(ul[i][j] * Bl[n][j] for j in range(R.RP)) for n in range(N)] for i in range(M)]
    assert torch.allclose(R.up64(u, B, y0, scale, drop), torch.tensor(up, dtype=F64), rtol=1e-13, atol=1e-14)
    assert torch.allclose(R.up64(u, B, y0.float(), scale, drop), torch.tensor(up, dtype=F64), rtol=1e-13, atol=1e-14)

    tn = [[scale * ks * sum(ul[i][j] * kx[i][k] * xl[i][k] for i in range(M)) for k in range(K)] for j in range(r)]
    want = torch.tensor(tn, dtype=F64)
    assert torch.allclose(R.tn64(u, x, r, scale, False, drop), want, rtol=1e-13, atol=1e-14)
    assert torch.equal(R.tn64(u, x, r, scale, True, drop), R.tn64(u, x, r, scale, False, drop).T)
    # without a mask: the plain products
    assert torch.equal(R.down64(x, P, 1.0), x.double() @ P.double().T)
    assert torch.equal(R.tn64(u, x, r, 1.0), (u.double().T @ x.double())[:r])


def test_the_mask_is_the_oracle_stream_taken_as_rows():
    d = R.Drop(0.25, 11, 7, 3, counter=5)
    for M, W in ((16, 32), (48, 160), (80, 288)):
        want = torch.from_numpy(philox.dropout_mask(M * W, 0.25, 11, 7, 8)).view(M, W)
        assert torch.equal(R.mult(M, W, d), want)
        assert torch.equal(R.keep(M, W, d), (want != 0).double())
        wide = torch.from_numpy(philox.dropout_mask(M * (W + 8), 0.25, 11, 7, 8)).view(M, W + 8)[:, :W]
        assert torch.equal(R.mult(M, W, d, W + 8), wide) and not torch.equal(wide, want)
    assert R.mult(16, 32, d).max().item() == philox.dropout_scale(0.25)
    assert torch.equal(R.mult(4, 8, R.NO_DROP), torch.ones(4, 8))
    assert R.scale32(0.75, d) == float(torch.tensor(0.75) * torch.tensor(float(philox.dropout_scale(0.25))))


def test_pack_reference_places_rounds_and_pads():
    for r, n_in, n_out in R.PACK_CASES:
        A, B = R.pack_inputs(r, n_in, n_out)
        A16, At16, B16, Bt16 = R.pack_ref(A, B)
        assert A16.shape == (16, n_in) and At16.shape == (n_in, 16) and B16.shape == (n_out, 16) and Bt16.shape == (16, n_out)
        assert torch.equal(A16[:r], A.bfloat16()) and bool((A16[r:] == 0).all()) and torch.equal(At16, A16.T)
        assert torch.equal(B16[:, :r], B.bfloat16()) and bool((B16[:, r:] == 0).all()) and torch.equal(Bt16, B16.T)
        # the ties are there and go to even, both ways
        assert A.view(-1)[0].item() == 1 + 2.0 ** -8 and A16.view(-1)[0].item() == 1.0
        assert A.view(-1)[1].item() == 1 + 3 * 2.0 ** -8 and A16.view(-1)[1].item() == 1 + 2.0 ** -6
        assert bool(torch.isfinite(A16.float()).all()) and bool(torch.isfinite(B16.float()).all())


def test_halfulp_bf16():
    v = torch.tensor([1.0, 1.99, 2.0, 0.75, 0.0, 300.0])
    assert R.halfulp_bf16(v).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0, 1.0]
    x = torch.tensor([1 + 2.0 ** -8 - 2.0 ** -20])                           # just under a tie: rounds down by almost half an ulp
    assert abs(x.bfloat16().double() - x.double()).item() <= R.halfulp_bf16(x).item()


@pytest.mark.parametrize('name', IDS)
def test_stand_in_is_fp32_noise(name):
    """A sanity rail for the stand-in only (no gate for a device): its fp32 value inside 2^-22 S of the float64 reference per rounding step
    it takes beyond the first -- at most 2 MFMAs per wave, the wave and slab sums, the scales: 8 steps -- so that no bound grows past
    8 x that; and its bf16 result inside what a device is allowed."""
    c = R.BY_NAME[name]
    n, b = R.noise(name), R.bound(c)
    print(name, f'stand-in {n:.2e}  bound {b:.2e}')
    assert n <= 8 * R.FLOOR
    assert R.FLOOR <= b <= 64 * R.FLOOR
    assert R.excess(R.stand_in(c), R.reference(c), R.scale(c), b, c.bf16_out) <= 1.0
    assert bool((R.scale(c) > 0).all())


@pytest.mark.parametrize('name', EXACT_IDS)
def test_exact_cases_are_exact(name):
    c = R.BY_NAME[name]
    inp = R.make_inputs(name)
    for t in inp.values():
        assert bool((t.float().abs() <= 2).all()) and bool((t.float() == t.float().round()).all())
    assert c.drop.p in (0.0, 0.5) and R.scale32(c.scale, c.drop) == c.scale * (2.0 if c.drop.p else 1.0)
    ref, pre, sin = R.reference(c), R.stand_in_f32(c), R.stand_in(c)
    assert torch.equal(pre.double(), ref)                                    # every partial sum and the result: exact in fp32
    assert torch.equal(sin.double(), ref)                                    # ... and the stored result (bf16 for down / up onto bf16 rows)
    assert R.same_bits(sin.double(), ref)                                    # (no -0.0 against +0.0 either)
    assert sin.dtype == (torch.bfloat16 if c.bf16_out else torch.float32)
    assert ref.abs().max().item() >= 8 and len(ref.unique()) >= 16           # (not a degenerate result)
    if c.drop.p:
        k = R.keep(c.M, c.W, c.drop)
        assert 0.4 < k.mean().item() < 0.6


def _caught(c, mutant):
    """How far outside the allowed error the mutant lies, in units of it (exact case: inf when any bit differs, else 0)."""
    ref, mut = R.reference(c), R.reference(c, mutant)
    if c.exact:
        return float('inf') if not torch.equal(mut, ref) else 0.0
    return R.excess(mut, ref, R.scale(c), R.bound(c), c.bf16_out)


@pytest.mark.parametrize('launch', ['down', 'up', 'tn'])
def test_every_mutant_is_caught_on_every_case_it_applies_to(launch):
    """Teeth: a random case must see the mutant at least twice as far out as a device may be (so that the rounding of a faulty device's own
    bf16 store cannot bring it back inside), an exact case must see a changed bit."""
    for mutant, what in R.MUTANTS[launch].items():
        cases = [c for c in R.of(launch) if R.mutant_applies(mutant, c)]
        assert [c for c in cases if not c.exact] and [c for c in cases if c.exact], (mutant, 'needs a random and an exact case')
        worst = {}
        for c in cases:
            e = _caught(c, mutant)
            worst[c.name] = e
            assert e >= 2.0, (mutant, what, c.name, e)
        finite = [e for e in worst.values() if e != float('inf')]
        print(f'{launch} {mutant}: {len(cases)} cases, outside by {min(finite):.0f} .. {max(finite):.0f} x the allowed error')
    for c in R.of(launch):                                                   # a mutant that does not apply leaves the case alone
        for mutant in R.MUTANTS[launch]:
            if not R.mutant_applies(mutant, c):
                assert torch.equal(R.reference(c, mutant), R.reference(c)), (mutant, c.name)


def test_masked_tn_cases_make_every_quad_exchange_matter():
    """Every masked case has kept and dropped elements; every masked tn case has both in EVERY 4 x 4 block (rows 4a..4a+3, columns 4b..4b+3)
    the quad exchange of lora_tn_kernel passes around."""
    seen = 0
    for c in R.ALL_CASES:
        if c.drop.p <= 0:
            continue
        k = R.keep(c.M, c.W, c.drop)
        assert 0 < k.mean().item() < 1, c.name
        assert c.drop.stream_id != 0 and c.drop.offset != 0
        if c.launch == 'tn':
            blocks = k.view(c.M // 4, 4, c.W // 4, 4).sum((1, 3))
            assert bool(((blocks > 0) & (blocks < 16)).all()), (c.name, 'a 4 x 4 mask block is all kept or all dropped: choose another seed')
            seen += 1
    assert seen >= 8


def test_the_case_lists_reach_every_cut():
    down, up, tn = (R.of(l, exact=False) for l in ('down', 'up', 'tn'))
    assert {c.M for c in down} == {16, 48} and {c.W for c in down} == {32, 96, 128, 160} and {c.pad for c in down} == {0, 8}
    assert {c.drop.p for c in down} == {0.0, 0.25} and any(c.W == 160 and c.pad and c.drop.p for c in down)
    assert {c.M for c in up} == {16, 80} and {c.W for c in up} == {32, 256, 288} and {c.pad for c in up} == {0, 8}
    assert {(c.f32, c.drop.p > 0) for c in up} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c.M for c in tn} == {32, 96, 256, 288, 544} and {c.W for c in tn} == {16, 48, 64, 80, 144} and {c.r for c in tn} == {1, 4, 7, 16}
    assert {(c.transpose, c.drop.p > 0) for c in tn} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c.pad for c in tn} == {0, 8} and any(c.M > 256 and c.drop.p for c in tn)
    for cases in (down, up, tn):
        assert sum(1 for c in cases if c.drop.counter) == 1 and 8 <= len(cases) <= 14
    for launch in ('down', 'up', 'tn'):
        ex = R.of(launch, exact=True)
        assert {c.drop.p for c in ex} == {0.0, 0.5}
    assert {c.f32 for c in R.of('up', exact=True)} == {False, True}
    for c in R.ALL_CASES:                                                    # what the library takes (lora.hip:227, :237, :258)
        assert c.M % (32 if c.launch == 'tn' else 16) == 0 and c.W % (16 if c.launch == 'tn' else 32) == 0 and c.pad % 8 == 0
    # rank entries 8..15 of U and the rank columns beyond r are non-zero
    for c in up + tn:
        assert bool((R.make_inputs(c.name)['u'].float() != 0).all())
    assert R.PACK_CASES == [(1, 8, 24), (7, 64, 192), (16, 32, 96)]
