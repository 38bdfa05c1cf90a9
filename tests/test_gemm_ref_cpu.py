"""tests/gemm_ref.py before anything is tied to it: the product model against plain float64 matmul and hand-made values, the hi / lo split's
exactness, the fp32 stand-in inside a sanity rail on every case, every mutant leaving the float64 reference by at least twice the bound a
device is held to, and the restated dispatch naming every instantiation tests/test_gpu_gemm_f64.py is there for.  No GPU."""
import pytest
import torch

import gemm_ref as R
from oracle import philox

F32, F64 = torch.float32, torch.float64
CASE_MODES = [(c.name, m) for c in R.CASES for m in c.modes]
IDS = [f'{n}-{m}' for n, m in CASE_MODES]


def _epilogues(case):
    return case.epilogues or [None]


def test_exact_in_float64_is_the_plain_product():
    case = R.BY_NAME['f32_65x67x33']
    inp = R.make_inputs(case.name)
    for mode in case.modes:                      # halo_gemm_f32 is exact in every math mode
        assert torch.equal(R.product64(case, mode, inp), inp['a'].double() @ inp['b'].double().T)
    a = torch.tensor([[1.0 + 2.0 ** -8, 3.0]]); b = torch.tensor([[1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0]])      # bf16: 8 significant bits
    assert R.rb(a)[0, 0].item() == 1.0 and R.rb(b)[0, 0].item() == 1.0 + 2.0 ** -6      # ties to even, both ways
    assert R.rb(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -9]), trunc=True).item() == 1.0
    c = R.Case('split', 1, 1, 2, R.SPLIT_MODES)
    exact = (1.0 + 2.0 ** -8) * (1.0 + 2.0 ** -7 + 2.0 ** -8) + 3.0
    assert R.product64(c, 'bf16', {'a': a, 'b': b}).item() == 1.0 * (1.0 + 2.0 ** -6) + 3.0
    assert R.product64(c, 'bf16x3', {'a': a, 'b': b}).item() == exact + 2.0 ** -16          # all but lo(a) lo(b) = -2^-8 * 2^-8
    assert [tuple(t[0].flatten().tolist()) for t in R.terms(c, 'bf16x3', {'a': a, 'b': b})] == [(2.0 ** -8, 0.0), (1.0, 3.0), (1.0, 3.0)]


def test_the_split_is_exact():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-90, 90, (1 << 16,), generator=g).float())
    hi, lo = R.split(x)
    assert torch.equal(hi, x.bfloat16().float()) and torch.equal(lo, (x - hi).bfloat16().float())
    assert torch.equal((hi + lo).double(), hi.double() + lo.double())                     # hi + lo is exact in fp32
    assert ((x.double() - hi.double() - lo.double()).abs() < 2.0 ** -16 * x.double().abs()).all()


def test_dropout_at_is_the_oracle_stream_at_those_elements():
    want = torch.from_numpy(philox.dropout_mask(5000, 0.3, R.SEED, R.STREAM_ID, R.OFFSET + 4))
    idx = torch.tensor([[0, 1, 2, 3], [4, 7, 4998, 4999], [1001, 1002, 2047, 2048]])
    assert torch.equal(R.dropout_at(idx, 0.3, offset=R.OFFSET + 4), want[idx])
    assert 0 < (want == 0).float().mean() < 1 and want.max().item() == philox.dropout_scale(0.3)


def test_row_sample_covers_the_tile_edges():
    case = R.BY_NAME['split_2100x2000x72']
    rows = set(R.sample_rows(case).tolist())
    for r0 in range(0, 2100, 128):
        assert {r0, min(r0 + 127, 2099)} <= rows and (r0 + 64 >= 2100 or {r0 + 63, r0 + 64} <= rows)
        assert len(rows & set(range(r0, r0 + 128))) >= (4 if r0 + 128 <= 2100 else 2)
    assert R.sample_rows(R.BY_NAME['split_256x128x2048']) is None


@pytest.mark.parametrize('name,mode', CASE_MODES, ids=IDS)
def test_stand_in_is_fp32_noise(name, mode):
    """A sanity rail for the stand-in only (no gate for a device): inside 2^-22 S sqrt(K) of the float64 reference on every case and
    epilogue set, so that no bound grows past 8 x that."""
    case = R.BY_NAME[name]
    rail = 2.0 ** -22 * case.K ** 0.5
    if case.entry == 'ce':
        ce = R.ce_reference(name, mode)
        print(name, mode, f"logits bound {ce['bound_logits']:.2e}  loss / lse bound {ce['bound_rows']:.2e}")
        assert ce['bound_logits'] <= R.FACTOR * rail and ce['bound_rows'] <= R.FACTOR * rail
        return
    for epi in (case.epilogues or [R.EPI_BY_NAME['bias1'], R.EPI_BY_NAME['bias1_residual']]):
        n = R.noise(name, mode, epi.name)
        print(name, mode, epi.name, f'stand-in {n:.2e}  bound {R.bound(name, mode, epi.name):.2e}')
        assert n <= rail, (epi.name, n, rail)
    for scratch in ((0,) if R.core(name, mode)['plan'].ksplit > 1 else ()):              # the unsplit form the GPU test also runs
        assert R.core(name, mode, scratch)['plan'].ksplit == 1
        assert R.noise(name, mode, 'bias1_accumulate', scratch) <= rail


@pytest.mark.parametrize('name,mode', CASE_MODES, ids=IDS)
def test_every_mutant_leaves_the_reference_by_twice_the_bound(name, mode):
    case, inp = R.BY_NAME[name], R.make_inputs(name)
    rows = R.core(name, mode)['rows']
    seen = set()
    for epi in (case.epilogues or [R.CE_EPI if case.entry == 'ce' else R.EPI_BY_NAME['bias1']]):
        pl = R.case_plan(case, mode, epi) if case.entry in ('f32', 'split') else R.core(name, mode)['plan']
        if case.entry == 'ce':
            bound = R.ce_reference(name, mode)['bound_logits']
        else:
            bound = R.bound(name, mode, epi.name)
        S = R.scale(case, epi, inp, rows)
        ref = R.reference(name, mode, epi)
        for mutant in R.MUTANTS:
            if not R.mutant_applies(mutant, case, mode, epi, pl):
                continue
            seen.add(mutant)
            dev = R.deviation(R.reference(name, mode, epi, mutant=mutant), ref, S)
            print(name, mode, epi.name, mutant, f'{dev:.2e} = {dev / bound:.0f} x bound')
            assert dev >= 2.0 * bound, (epi.name, mutant, dev, bound)
    assert 'last_ktile_dropped' in seen


def test_the_case_table_reaches_every_instantiation():
    """plan() over the case table: what tests/test_gpu_gemm_f64.py then checks really ran (the lent scratch's contents)."""
    labels = set()
    for c in R.CASES:
        for mode in c.modes:
            if c.entry in ('io', 'ioout'):
                for f in (R.A_ROWMAJOR, R.A_ROWMAJOR | R.ACCUM, R.OUT_BF16, R.OUT_BF16 | R.GELU):
                    labels.add(R.plan('io', mode, c.M, c.N, c.K, f).label)
                continue
            for epi in _epilogues(c):
                labels.add(R.case_plan(c, mode, epi).label)
    print(sorted(labels))
    want = {'f32 64x64', 'f32 128x128', 'f32 64x64 + vector reduce', 'f32 64x64 + scalar reduce', 'f32 128x128 + vector reduce'}
    want |= {f'x3 two-slot {e}' for e in ('lean', 'lean-add', 'full')} | {'x3 two-slot slice + vector reduce', 'x3 two-slot slice + scalar reduce'}
    want |= {f'x3 one-slot {e}' for e in ('lean', 'lean-add', 'full')}
    want |= {f'bf16 three-slot {e}' for e in ('lean', 'lean-add', 'full')} | {'bf16 three-slot slice + vector reduce', 'bf16 three-slot slice + scalar reduce'}
    want |= {'bf16 half-tile lean', 'bf16 half-tile lean-add'}
    want |= {f'{r} {e} io A row-major' for r in ('x3 two-slot', 'bf16 three-slot') for e in ('lean', 'lean-add')}
    want |= {f'{r} {e} io bf16 out' for r in ('x3 two-slot', 'bf16 three-slot') for e in ('lean', 'full')}
    want |= {'x3 two-slot ce', 'x3 one-slot ce', 'bf16 three-slot ce'}
    assert want <= labels, want - labels


def test_plan_restates_the_slicing_of_the_named_cases():
    P = R.plan
    p = P('f32', 'f32', 70, 33, 1000)
    assert (p.tile, p.ksplit, p.kper, p.reduce) == ((64, 64), 8, 128, 'scalar') and 1000 - 7 * 128 == 104
    p = P('f32', 'f32', 1800, 1700, 2048)
    assert (p.tile, p.ntiles, p.ksplit, p.kper, p.reduce) == ((128, 128), 210, 2, 1024, 'vector')
    assert P('f32', 'f32', 1800, 1700, 2048, scratch_bytes=0).ksplit == 1
    p = P('split', 'bf16x3', 256, 128, 2048)
    assert (p.ksplit, p.ktper, p.reduce) == (16, 4, 'vector')
    p = P('split', 'bf16', 200, 130, 2100)
    assert (p.ksplit, p.ktper, p.reduce) == (14, 5, 'scalar') and 66 - 13 * 5 == 1
    p = P('split', 'bf16x3', 1536, 1280, 2048)
    assert (p.ntiles, p.ksplit, p.ktper) == (120, 3, 22)
    p = P('split', 'bf16x3', 4100, 3080, 40, R.GELU)
    assert (p.ntiles, p.ksplit, p.label) == (825, 1, 'x3 one-slot full')
    p = P('split', 'bf16', 2100, 2000, 72, R.ACCUM)
    assert (p.tile, p.ntiles, p.label) == ((64, 128), 33 * 16, 'bf16 half-tile lean-add') and 2100 - 32 * 64 == 52
    assert P('split', 'bf16', 2100, 2000, 72, R.ACCUM, half_tiles=False).label == 'bf16 three-slot lean-add'
    assert P('split', 'bf16', 2100, 2000, 72, R.RELU).label == 'bf16 three-slot full'           # the half tiles: lean epilogues only
    assert P('split', 'bf16x3', 2100, 2000, 72).label == 'x3 two-slot lean'                     # ... and single pass only
    assert P('split', 'bf16', 130, 70, 96, R.DROP | R.ACCUM).label == 'bf16 three-slot full'
