"""The GEMM core (csrc/gemm_f32.hip, csrc/gemm_bf16x3.hip, the operand-image builders of csrc/tiled_image.h) against float64 under each math
mode's own operand rounding (tests/gemm_ref.py; DESIGN.md "GEMM against float64"), per dispatched instantiation.

Every case x mode x epilogue set is held to max(8 x the fp32 stand-in's own deviation from the float64 reference, 2^-22) in units of the
per-element scale S; the lent split-K scratch shows which plan ran; the operand images are decoded bit for bit; the dropout multipliers are
the oracle's."""
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PATTERN = 0x7fc00abc              # a quiet NaN with a payload: what the lent scratch holds before a call


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, ops
    _lib.lib()
    sc = _lib.lend_scratch()
    _lib.check(_lib.lib().halo_set_scratch(sc.data_ptr(), sc.numel()), 'halo_set_scratch')
    return dict(ops=ops, lib=_lib, scratch=sc)


class _Mode:
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.get_math_mode()
        self.lib.set_math_mode(self.mode)

    def __exit__(self, *exc):
        self.lib.set_math_mode(self.prev)


_dev_cache = {}


def _dev(name):
    """The device copies of a case's inputs, built once per case (one case is held at a time)."""
    if name not in _dev_cache:
        _dev_cache.clear()
        _dev_cache[name] = {k: v.to(DEV) for k, v in R.make_inputs(name).items()}
    return _dev_cache[name]


def _poison(hal):
    hal['scratch'].view(torch.int32).fill_(PATTERN)


def _scratch_holds(hal, n):
    """Exactly the first n floats of the lent scratch were written (with finite values); the rest still holds the pattern."""
    f = hal['scratch'].view(torch.float32)
    assert bool(torch.isfinite(f[:n]).all()), 'a slab element the plan names was not written'
    assert bool((hal['scratch'].view(torch.int32)[n:] == PATTERN).all()), 'the scratch was written past the plan\'s slabs'


def _drop(hal, epi):
    return hal['ops'].Dropout(epi.p, R.SEED, R.OFFSET) if epi.p > 0 else hal['ops'].NO_DROPOUT


def _report(name, mode, labels, ratios):
    print(f'\n{name} [{mode}] device/bound ' + '  '.join(f'{k} {v:.2f} ({labels[k]})' for k, v in ratios.items()))


def _kw(d, epi):
    return dict(bias1=d['bias1'] if epi.bias1 else None, bias2=d['bias2'] if epi.bias2 else None, relu=epi.relu, gelu=epi.gelu)


def _hold(case, mode, epi, got_dev, scratch_bytes, failures, ratios, key=None, stand_in_too=False):
    """got_dev [M, N] on the device against the float64 reference on the case's row sample."""
    rows = R.core(case.name, mode, scratch_bytes)['rows']
    got = (got_dev if rows is None else got_dev[rows.to(DEV)]).cpu()
    inp = R.make_inputs(case.name)
    ref = R.reference(case.name, mode, epi, scratch_bytes)
    S = R.scale(case, epi, inp, rows)
    bound = R.bound(case.name, mode, epi.name, scratch_bytes)
    dev = R.deviation(got, ref, S)
    ratios[key or epi.name] = dev / bound
    if not dev <= bound:
        failures.append((key or epi.name, dev, bound, 'first (row, col, device, reference):', R.first_outside(got, ref, S, bound, rows)))
    if stand_in_too:
        # the documented bit-exact model of the f32 MFMA: only double rounding in the emulated fma separates the two
        sin = R.stand_in(case.name, mode, epi, scratch_bytes)
        d2 = R.deviation(got, sin, S)
        if not d2 <= R.FLOOR:
            failures.append((key or epi.name, 'against the fp32 stand-in', d2, R.FLOOR, R.first_outside(got, sin, S, R.FLOOR, rows)))


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gemm_f32
# ------------------------------------------------------------------------------------------------------------------------------
F32_CASES = [(c, m, akc, bkc) for c in R.CASES if c.entry == 'f32' for m in c.modes for akc, bkc in ((1, 1), (1, 0), (0, 0), (0, 1))]


def _f32_operands(d, akc, bkc):
    return (d['a'] if akc else d['a'].t().contiguous()), (d['b'] if bkc else d['b'].t().contiguous())


def _run_f32(hal, case, d, A, B, akc, bkc, epi):
    out = d['addend'].clone() if epi.addend else None
    return hal['ops'].gemm(A, B, akc, bkc, case.M, case.N, case.K, out=out, drop=_drop(hal, epi), stream_id=R.STREAM_ID,
                           accumulate=bool(epi.addend), **_kw(d, epi))


@pytest.mark.parametrize('case,mode,akc,bkc', F32_CASES, ids=[f'{c.name}-{m}-a{a}b{b}' for c, m, a, b in F32_CASES])
def test_gemm_f32_matches_float64_per_instantiation(hal, case, mode, akc, bkc):
    """Observed device/bound ratios: DESIGN.md "GEMM against float64"."""
    d = _dev(case.name)
    nbytes = hal['scratch'].numel()
    failures, ratios, labels = [], {}, {}
    with _Mode(hal['lib'], mode):
        A, B = _f32_operands(d, akc, bkc)
        for epi in case.epilogues:
            pl = R.case_plan(case, mode, epi, nbytes)
            labels[epi.name] = pl.label
            _poison(hal)
            got = _run_f32(hal, case, d, A, B, akc, bkc, epi)
            _scratch_holds(hal, pl.ksplit * case.M * case.N if pl.ksplit > 1 else 0)
            _hold(case, mode, epi, got, nbytes, failures, ratios, stand_in_too=not (epi.relu or epi.gelu))
    _report(case.name, mode, labels, ratios)
    assert not failures, failures


@pytest.mark.parametrize('akc,bkc', [(1, 1), (1, 0), (0, 0), (0, 1)])
def test_gemm_f32_from_misaligned_views_equals_the_aligned_run(hal, akc, bkc):
    """Operands read from views buf[:, 1:1+n] of wider buffers (a base that is no multiple of 16 bytes: a_vec = b_vec = 0, scalar loads) give
    the bits of the aligned run (the k order is the same), whose float64 gate is the test above."""
    case = R.BY_NAME['f32_96x64x64']
    d = _dev(case.name)
    A, B = _f32_operands(d, akc, bkc)

    def view(t):
        buf = torch.full((t.shape[0], t.shape[1] + 8), float('nan'), device=DEV)
        buf[:, 1:1 + t.shape[1]] = t
        v = buf[:, 1:1 + t.shape[1]]
        assert v.data_ptr() % 16 == 4 and v.stride(0) % 4 == 0
        return v

    for epi in (R.EPI_BY_NAME['plain'], R.EPI_BY_NAME['bias12_relu'], R.EPI_BY_NAME['bias1_gelu_drop_accumulate']):
        want = _run_f32(hal, case, d, A, B, akc, bkc, epi)
        assert torch.equal(_run_f32(hal, case, d, view(A), view(B), akc, bkc, epi), want), epi.name
        assert torch.equal(_run_f32(hal, case, d, view(A), B, akc, bkc, epi), want), epi.name


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gemm_split / halo_gemm_split_residual
# ------------------------------------------------------------------------------------------------------------------------------
SPLIT_CASES = [(c, m) for c in R.CASES if c.entry == 'split' for m in c.modes]


def _run_split(hal, case, d, ai, bi, epi):
    out = d['addend'].clone() if epi.addend == 'accumulate' else None
    return hal['ops'].gemm_split(ai, bi, case.M, case.N, case.K, out=out, drop=_drop(hal, epi), stream_id=R.STREAM_ID,
                                 accumulate=epi.addend == 'accumulate', residual=d['addend'] if epi.addend == 'residual' else None, **_kw(d, epi))


@pytest.mark.parametrize('case,mode', SPLIT_CASES, ids=[f'{c.name}-{m}' for c, m in SPLIT_CASES])
def test_gemm_split_matches_float64_per_instantiation(hal, monkeypatch, case, mode):
    """Observed device/bound ratios: DESIGN.md "GEMM against float64"."""
    if not case.half_tiles:
        monkeypatch.setenv('HALO_GEMM_HALF_TILES', '0')
    else:
        monkeypatch.delenv('HALO_GEMM_HALF_TILES', raising=False)
    d = _dev(case.name)
    nbytes = hal['scratch'].numel()
    failures, ratios, labels = [], {}, {}
    with _Mode(hal['lib'], mode):
        ai, bi = hal['ops'].split_image(d['a']), hal['ops'].split_image(d['b'])
        for epi in case.epilogues:
            pl = R.case_plan(case, mode, epi, nbytes)
            labels[epi.name] = pl.label
            _poison(hal)
            got = _run_split(hal, case, d, ai, bi, epi)
            _scratch_holds(hal, pl.ksplit * case.M * case.N if pl.ksplit > 1 else 0)
            _hold(case, mode, epi, got, nbytes, failures, ratios)
    _report(case.name, mode, labels, ratios)
    assert not failures, failures


UNSPLIT = [(c, m) for c in R.CASES if c.entry in ('f32', 'split') for m in c.modes[:2] if R.case_plan(c, m).ksplit > 1]


@pytest.mark.parametrize('case,mode', UNSPLIT, ids=[f'{c.name}-{m}' for c, m in UNSPLIT])
def test_without_scratch_the_split_k_cases_run_whole_and_meet_the_unsplit_bound(hal, case, mode):
    lib = hal['lib']
    d = _dev(case.name)
    failures, ratios, labels = [], {}, {}
    assert R.case_plan(case, mode, None, 0).ksplit == 1
    with _Mode(lib, mode):
        _poison(hal)
        lib.check(lib.lib().halo_set_scratch(None, 0), 'halo_set_scratch')
        try:
            for epi in (R.EPI_BY_NAME['bias1_accumulate'], R.EPI_BY_NAME['bias1_gelu_drop_accumulate']):
                labels[epi.name] = R.case_plan(case, mode, epi, 0).label
                if case.entry == 'f32':
                    got = _run_f32(hal, case, d, d['a'], d['b'], 1, 1, epi)
                else:
                    got = _run_split(hal, case, d, hal['ops'].split_image(d['a']), hal['ops'].split_image(d['b']), epi)
                _hold(case, mode, epi, got, 0, failures, ratios)
        finally:
            lib.check(lib.lib().halo_set_scratch(hal['scratch'].data_ptr(), hal['scratch'].numel()), 'halo_set_scratch')
        _scratch_holds(hal, 0)
    _report(case.name + ' (no scratch)', mode, labels, ratios)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gemm_split_io
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.SPLIT_MODES)
def test_gemm_split_io_rowmajor_a_takes_the_given_parts(hal, mode):
    """A as a row-major (hi, lo) pair cut out of wider buffers (lda = K + 8, NaN beside the rows): the product of exactly those parts."""
    case = R.BY_NAME['io_300x224x96']
    d = _dev(case.name)
    ops = hal['ops']
    M, N, K = case.M, case.N, case.K
    failures, ratios, labels = [], {}, {}

    def cut(t):
        buf = torch.full((M, K + 8), float('nan'), device=DEV, dtype=torch.bfloat16)
        buf[:, :K] = t
        return buf[:, :K]

    with _Mode(hal['lib'], mode):
        a = (cut(d['a_hi']), cut(d['a_lo']) if mode == 'bf16x3' else None)
        bi = ops.split_image(d['b'])
        for epi in (R.EPI_BY_NAME['bias1'], R.EPI_BY_NAME['bias1_residual'], R.EPI_BY_NAME['bias1_accumulate']):
            labels[epi.name] = R.plan('io', mode, M, N, K, R.A_ROWMAJOR | epi.flags).label
            _poison(hal)
            got = ops.gemm_split_io(a, bi, M, N, K, out=d['addend'].clone() if epi.addend == 'accumulate' else None, bias1=d['bias1'],
                                    accumulate=epi.addend == 'accumulate', residual=d['addend'] if epi.addend == 'residual' else None)
            _scratch_holds(hal, 0)
            _hold(case, mode, epi, got, R.SCRATCH, failures, ratios)
    _report(case.name, mode, labels, ratios)
    assert not failures, failures


@pytest.mark.parametrize('mode', R.SPLIT_MODES)
def test_gemm_split_io_bf16_output_is_the_split_of_the_fp32_result(hal, mode):
    case = R.BY_NAME['ioout_300x224x96']
    d = _dev(case.name)
    ops = hal['ops']
    M, N, K = case.M, case.N, case.K
    failures, ratios, labels = [], {}, {}
    with _Mode(hal['lib'], mode):
        ai, bi = ops.split_image(d['a']), ops.split_image(d['b'])
        for epi in (R.EPI_BY_NAME['bias1'], R.EPI_BY_NAME['bias1_gelu']):
            labels[epi.name] = R.plan('io', mode, M, N, K, R.OUT_BF16 | epi.flags).label
            c = torch.empty(M, N, device=DEV)
            hi, lo = ops.gemm_split_io(ai, bi, M, N, K, out=c, out_rowmajor=True, bias1=d['bias1'], gelu=epi.gelu)
            assert torch.equal(hi, c.bfloat16()), epi.name
            if mode == 'bf16x3':
                assert torch.equal(lo, (c - hi.float()).bfloat16()), epi.name
            else:
                assert lo is None
            hi2, lo2 = ops.gemm_split_io(ai, bi, M, N, K, out_rowmajor=True, bias1=d['bias1'], gelu=epi.gelu)      # no fp32 written
            assert torch.equal(hi2, hi) and (lo is None or torch.equal(lo2, lo)), epi.name
            _hold(case, mode, epi, c, R.SCRATCH, failures, ratios)
    _report(case.name, mode, labels, ratios)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------------
# halo_gemm_split_ce
# ------------------------------------------------------------------------------------------------------------------------------
CE_CASES = [(c, m) for c in R.CASES if c.entry == 'ce' for m in c.modes]


@pytest.mark.parametrize('case,mode', CE_CASES, ids=[f'{c.name}-{m}' for c, m in CE_CASES])
def test_gemm_split_ce_matches_float64_cross_entropy(hal, case, mode):
    """loss, lse and the optional logits against the float64 cross-entropy of the reference logits (targets in the last ragged 64-column strip,
    every seventh row ignored).  Observed device/bound ratios: DESIGN.md "GEMM against float64"."""
    d = _dev(case.name)
    ops = hal['ops']
    M, N, K = case.M, case.N, case.K
    ce = R.ce_reference(case.name, mode)
    rows = ce['rows']
    pick = (lambda t: t.cpu()) if rows is None else (lambda t: t[rows.to(DEV)].cpu())
    with _Mode(hal['lib'], mode):
        ai, bi = ops.split_image(d['a']), ops.split_image(d['b'])
        _poison(hal)
        loss, lse, logits = ops.gemm_split_ce(ai, bi, M, N, K, d['targets'], ignore_index=R.IGNORE_INDEX, bias=d['bias1'], want_logits=True, want_lse=True)
        loss2, none, none2 = ops.gemm_split_ce(ai, bi, M, N, K, d['targets'], ignore_index=R.IGNORE_INDEX, bias=d['bias1'])
        _scratch_holds(hal, 0)
    assert none is None and none2 is None and torch.equal(loss2, loss)
    ignored = d['targets'] == R.IGNORE_INDEX
    assert bool(ignored[::7].all()) and bool((loss[ignored] == 0).all()) and bool((lse[ignored] == 0).all())
    got = pick(logits)
    dl = R.deviation(got, ce['logits'], ce['S'])
    d_loss = ((pick(loss).double() - ce['loss']).abs() / ce['unit']).max().item()
    d_lse = ((pick(lse).double() - ce['lse']).abs() / ce['unit']).max().item()
    label = R.case_plan(case, mode).label
    print(f"\n{case.name} [{mode}] {label}: device/bound logits {dl / ce['bound_logits']:.2f}  loss {d_loss / ce['bound_rows']:.2f}  "
          f"lse {d_lse / ce['bound_rows']:.2f}")
    assert dl <= ce['bound_logits'], (dl, ce['bound_logits'], R.first_outside(got, ce['logits'], ce['S'], ce['bound_logits'], rows))
    assert d_loss <= ce['bound_rows'], (d_loss, ce['bound_rows'])
    assert d_lse <= ce['bound_rows'], (d_lse, ce['bound_rows'])


# ------------------------------------------------------------------------------------------------------------------------------
# the operand images, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def _values(rows, cols, seed):
    """fp32 [rows, cols]: magnitudes from 1e-30 to 1e30, and up front exact ties at the bf16 rounding boundary (both parities, both signs, in
    hi and in lo), +-0 and the largest finite bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-100, 101, (rows, cols), generator=g).float())
    special = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),                  # ties in hi: to even, down and up
               1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9 + 3 * 2.0 ** -17, -(1 + 2.0 ** -9 + 2.0 ** -17),  # ties in lo = rb(x - 1)
               0.0, -0.0, 3.3895313892515355e38, -3.3895313892515355e38, (1 + 2.0 ** -8) * 2.0 ** -90, (1 + 3 * 2.0 ** -8) * 2.0 ** 90]
    flat = x.view(-1)
    n = min(len(special), flat.numel())
    flat[:n] = torch.tensor(special[:n])
    flat[-n:] = torch.tensor(special[:n])
    return x


def _sources():
    """name -> the source view on the device (values from _values)."""
    out = {}
    buf = torch.full((129, 41), float('nan'), device=DEV)
    buf[:, :33] = _values(129, 33, 1).to(DEV)
    out['129x33_stride41'] = buf[:, :33]
    out['128x64'] = _values(128, 64, 2).to(DEV)
    buf = torch.zeros(202 * 103, device=DEV)
    buf[::2] = float('nan')                                            # every other element NaN (an odd row length: a checkerboard)
    buf = buf.view(202, 103)
    buf[1:201, 1:101] = _values(200, 100, 3).to(DEV)
    out['200x100_in_nan'] = buf[1:201, 1:101]
    out['4x40'] = _values(4, 40, 4).to(DEV)
    return out


def _decode(ops, img, rows, k):
    """The values an image holds, through the product that reads it: x identity [k, k] (exact in bf16; hi + lo is exact in fp32)."""
    return ops.gemm_split(img, ops.split_image(torch.eye(k, device=DEV)), rows, k, k)


def _want(x, mode):
    hi, lo = R.split(x.cpu().contiguous())
    return hi + lo if mode == 'bf16x3' else hi


def _same(got, want, what):
    got = got.cpu()
    if not torch.equal(got, want):
        i = tuple(torch.nonzero(got != want)[0].tolist())
        raise AssertionError((what, 'first difference (index, image, wanted):', i, got[i].item(), want[i].item()))


@pytest.mark.parametrize('mode', R.SPLIT_MODES)
def test_every_image_builder_writes_the_split_of_its_source_bit_for_bit(hal, mode):
    ops = hal['ops']
    with _Mode(hal['lib'], mode):
        src = _sources()
        for name, x in src.items():
            r, k = x.shape
            _same(_decode(ops, ops.split_image(x), r, k), _want(x, mode), (name, 'split_image'))
            _same(_decode(ops, ops.split_image(x, transposed=True), k, r), _want(x.t(), mode), (name, 'split_image transposed'))
            rm, tr = ops.image_pair(x)
            _same(_decode(ops, rm, r, k), _want(x, mode), (name, 'image_pair rows'))
            _same(_decode(ops, tr, k, r), _want(x.t(), mode), (name, 'image_pair columns'))
            only_rm, none = ops.image_pair(x, cols_image=False)
            assert none is None
            _same(_decode(ops, only_rm, r, k), _want(x, mode), (name, 'image_pair rows only'))
        for (name, x), (rm, tr) in zip(src.items(), ops.image_pairs(list(src.values()))):
            r, k = x.shape
            _same(_decode(ops, rm, r, k), _want(x, mode), (name, 'image_pairs rows'))
            _same(_decode(ops, tr, k, r), _want(x.t(), mode), (name, 'image_pairs columns'))
        g = torch.Generator().manual_seed(9)
        for rows, C in ((128, 64), (130, 96), (4, 64)):                 # layernorm_image: contiguous rows of whole k-tiles
            x = (torch.randn(rows, C, generator=g) * 3 + 1).to(DEV)
            w, b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
            img, y = ops.layernorm_image(x, w, b, want_y=True)
            _same(_decode(ops, img, rows, C), _want(y, mode), ((rows, C), 'layernorm_image'))


def test_an_image_built_for_three_passes_read_in_one_gives_the_rounded_source(hal):
    ops, lib = hal['ops'], hal['lib']
    with _Mode(lib, 'bf16x3'):
        src = _sources()
        imgs = {n: (ops.split_image(x), ops.split_image(torch.eye(x.shape[1], device=DEV))) for n, x in src.items()}
        lib.set_math_mode('bf16')
        for n, x in src.items():
            r, k = x.shape
            _same(ops.gemm_split(imgs[n][0], imgs[n][1], r, k, k), _want(x, 'bf16'), n)


# ------------------------------------------------------------------------------------------------------------------------------
# dropout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,reduce', [('split_130x70x96', ''), ('split_256x128x2048', 'vector'), ('split_200x130x2100', 'scalar'),
                                         ('f32_65x67x33', ''), ('f32_70x33x1000', 'scalar')])
def test_dropout_multipliers_are_the_oracle_stream_at_offset_plus_counter(hal, name, reduce):
    """The fused epilogue, the vector reduce (four multipliers per Philox call) and the scalar reduce apply the oracle's multiplier of element
    row * N + col, drawn at offset + the device counter: with and without dropout the same launch differs by exactly that factor."""
    case = R.BY_NAME[name]
    mode = 'f32' if case.entry == 'f32' else 'bf16'
    d = _dev(name)
    ops = hal['ops']
    assert R.case_plan(case, mode, R.EPI_BY_NAME['bias1_gelu'], hal['scratch'].numel()).reduce == reduce
    counter = torch.tensor([4], dtype=torch.int32, device=DEV)
    drop = ops.Dropout(R.P_DROP, R.SEED, R.OFFSET, counter=counter)
    with _Mode(hal['lib'], mode):
        if case.entry == 'f32':
            run = lambda dr: ops.gemm(d['a'], d['b'], 1, 1, case.M, case.N, case.K, bias1=d['bias1'], gelu=True, drop=dr, stream_id=R.STREAM_ID)
        else:
            ai, bi = ops.split_image(d['a']), ops.split_image(d['b'])
            run = lambda dr: ops.gemm_split(ai, bi, case.M, case.N, case.K, bias1=d['bias1'], gelu=True, drop=dr, stream_id=R.STREAM_ID)
        with_drop, without = run(drop).cpu(), run(ops.NO_DROPOUT).cpu()
    m = R.dropout_at(torch.arange(case.M * case.N).view(case.M, case.N), R.P_DROP, offset=R.OFFSET + 4)
    assert counter.item() == 4 and 0.2 < (m == 0).float().mean().item() < 0.4
    assert torch.equal(with_drop, without * m)
