"""tests/rows_ref.py before anything is tied to it: the summation orders against plain loops, each float64 restatement against torch's own
operator, the exact cases exact (reference == stand-in bit for bit), the fp32 stand-in inside a rail on every random case, every mutant
outside what a device is allowed on every case listed for it, the tables reaching every dispatch edge, and every table entry consumed by
tests/test_gpu_rows_f64.py.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref
import rows_ref as R

F64 = torch.float64
RAIL = 4 * R.FLOOR
IDS = [c.name for c in R.ALL_CASES]


def test_the_constants():
    assert R.FLOOR is gemm_ref.FLOOR and (R.FACTOR, R.FLOOR, R.TINY) == (4.0, 2.0 ** -22, 2.0 ** -126)


# ------------------------------------------------------------------------------------------------------------------------------
# the orders
# ------------------------------------------------------------------------------------------------------------------------------
def test_wave_sum_is_the_butterfly_of_halo_common():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(3, 64, generator=g)
    want = []
    for row in v:
        lanes = [row[i] for i in range(64)]
        for n in (8, 4, 2, 1):                                               # row_ror:n inside each row of 16 lanes
            lanes = [lanes[i] + lanes[i // 16 * 16 + (i % 16 - n) % 16] for i in range(64)]
        lanes = [lanes[i] + lanes[i ^ 16] for i in range(64)]
        lanes = [lanes[i] + lanes[i ^ 32] for i in range(64)]
        assert all(R.same_bits(lanes[i], lanes[0]) for i in range(64))       # every lane ends with the same bits
        want.append(lanes[0])
    assert R.same_bits(R.wave_sum32(v), torch.stack(want))
    ints = torch.randint(-4, 5, (2, 64), generator=g).float()
    assert torch.equal(R.wave_sum32(ints), ints.sum(1))


@pytest.mark.parametrize('rows', [1, 31, 32, 33, 96, 97, 127, 128, 129, 225, 300])
def test_colsum32_walks_the_kernels_loop(rows):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 3, generator=g)
    part = torch.zeros(32, 3)
    for sl in range(32):
        s = [torch.zeros(3) for _ in range(4)]
        r = sl
        while r + 96 < rows:
            for j in range(4):
                s[j] = s[j] + x[r + 32 * j]
            r += 128
        while r < rows:
            s[0] = s[0] + x[r]
            r += 32
        part[sl] = (s[0] + s[1]) + (s[2] + s[3])
    t = torch.zeros(3)
    for sl in range(32):
        t = t + part[sl]
    assert R.same_bits(R.colsum32(x), t)


def test_lane_sum_and_fma():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 200, generator=g)
    lanes = torch.zeros(2, 64)
    for c in range(200):
        lanes[:, c % 64] = lanes[:, c % 64] + x[:, c]
    assert R.same_bits(R.lane_sum32(x), R.wave_sum32(lanes))
    a, b, c = (torch.randn(50, generator=g) for _ in range(3))
    assert torch.equal(R.fma32(a, b, c), (a.double() * b.double() + c.double()).float())


# ------------------------------------------------------------------------------------------------------------------------------
# the restatements against torch's operators
# ------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin) and torch.equal(a[~fin], b[~fin])
    assert torch.allclose(a[fin], b[fin], rtol=tol, atol=tol), (a[fin] - b[fin]).abs().max()


def test_layernorm_restatements_equal_autograd():
    for name in ('ln_fwd-C200_r37_b_wide', 'ln_fwd-C65_r1_nb_wide'):
        c, i = R.BY_NAME[name], R.make_inputs(name)
        want = F.layer_norm(i['x'].double(), (c.C,), i['w'].double(), None if i['b'] is None else i['b'].double(), float(R.f32(R.EPS)))
        _close(R.reference(c)['y'], want)
    for name in ('ln_bwd-C260_r5_nobias', 'ln_bwd-C8_r5', 'ln_bwd-C201_r5_nobias'):
        c, i = R.BY_NAME[name], R.make_inputs(name)
        x, w, b = i['x'].double().requires_grad_(), i['w'].double().requires_grad_(), torch.zeros(c.C, dtype=F64, requires_grad=True)
        F.layer_norm(x, (c.C,), w, b, float(R.f32(R.EPS))).backward(i['dy'].double())
        ref = R.reference(c)
        _close(ref['dx'], x.grad + (i['dres'].double() if i['dres'] is not None else 0))
        _close(ref['dw'], w.grad)
        if c.has_bias:
            _close(ref['db'], b.grad)


def test_cross_entropy_and_log_softmax_restatements_equal_torch():
    for c in R.CE:
        i = R.make_inputs(c.name)
        x = i['x'].double().requires_grad_()
        loss = F.cross_entropy(x, i['tgt'], ignore_index=c.ignore, reduction='none')
        ref = R.reference(c)
        _close(ref['loss'], loss.detach())
        live = i['tgt'] != c.ignore
        _close(ref['lse'][live], torch.logsumexp(x.detach(), 1)[live])
        assert bool((ref['lse'][~live] == 0).all()) and bool((ref['loss'][~live] == 0).all()) and int((~live).sum()) == 2
        assert bool(torch.isfinite(ref['lse']).all())                        # some logit of every row is finite
        gr = i['grad'].double().expand(c.rows)
        (loss * gr).sum().backward()
        exact_lse = torch.where(live, torch.logsumexp(x.detach(), 1), torch.zeros(c.rows, dtype=F64))
        _close(R.reference(c, lse=exact_lse)['dlogits'], x.grad)                # (the launch takes an fp32 lse as an input: here the exact one)
        assert (i['lse'].double() - exact_lse).abs().max() <= 2.0 ** -24 * exact_lse.abs().max()
        assert bool(((i['tgt'] >= 0) & (i['tgt'] < c.V) | ~live).all())      # the precondition: no target outside [0, V)
    for c in R.LSM_FWD:
        i = R.make_inputs(c.name)
        _close(R.reference(c)['y'], torch.log_softmax(i['x'].double(), 1))
    for c in R.LSM_BWD:
        i = R.make_inputs(c.name)
        y = i['y'].double()
        _close(R.reference(c)['dx'], i['dy'].double() - torch.exp(y) * i['dy'].double().sum(1, keepdim=True))
        assert (torch.exp(y).sum(1) - 1).abs().max() < 1e-5


def test_gelu_restatements_equal_torch():
    for c in R.GELU_FWD + R.GELU_BWD:
        i = R.make_inputs(c.name)
        a = i['a'].double().requires_grad_()
        y = F.gelu(a, approximate='tanh' if c.kind == 'tanh' else 'none')
        if c.launch == 'gelu_fwd':
            _close(R.reference(c)['y'], y.detach(), 1e-14)
        else:
            y.backward(i['dy'].double())
            _close(R.reference(c)['da'], a.grad, 1e-14)
    a = R.make_inputs('gelu_fwd-tanh_n255')['a']
    assert a.min() == -12 and a.max() >= 12 and int((a == 0).sum()) >= 2 and int(((a != 0) & (a.abs() < 2.0 ** -126)).sum()) >= 4


def test_embedding_restatements_equal_torch():
    for c in R.EMBED_FWD:
        i = R.make_inputs(c.name)
        ids = i['ids'].clamp(0, R.VOCAB - 1)
        want = F.embedding(ids, i['wte'].double()).view(-1, c.C)
        if c.wpe:
            want = want + F.embedding(c.pos0 + torch.arange(c.T), i['wpe'].double()).repeat(c.B, 1)
        _close(R.reference(c)['x'], want)
        assert int(i['ids'].max()) == R.VOCAB + 2 and (c.B * c.T == 1 or int(i['ids'].min()) == -3)
    for c in R.EMBED_BWD + R.EMBED_ORD:
        i = R.make_inputs(c.name)
        ids = i['ids'].view(-1).clamp(0, R.VOCAB - 1)
        ref = R.reference(c)
        if 'dwte' in ref:
            base = i['dwte0'].double() if c.launch == 'embed_bwd' else torch.zeros(R.VOCAB, c.C, dtype=F64)
            _close(ref['dwte'], base.index_add(0, ids, i['dx'].double()), 1e-13)
            absent = [v for v in range(R.VOCAB) if v not in ids.tolist()]
            assert absent and (c.launch != 'embed_ord' or bool((ref['dwte'][absent] == 0).all()))
        if 'dwpe' in ref:
            want = i['dwpe0'].double().clone()
            s = i['dx'].double().view(c.B, c.T, c.C).sum(0)
            want[c.pos0:c.pos0 + c.T] = want[c.pos0:c.pos0 + c.T] + s if c.acc else s
            _close(ref['dwpe'], want, 1e-13)


def test_conv_restatements_equal_torch():
    for c in R.IM2COL:
        x = R.make_inputs(c.name)['x']
        ref = R.reference(c)['col']
        assert R.same_bits(ref.float(), R.im2col_unfold(c, x)) and torch.equal(ref.float().double(), ref)       # a pure copy
    for c in R.COL2IM:
        d = R.make_inputs(c.name)['dcol'].double()
        To = R.conv_out(c.T, c.ks, c.stride, c.pad)
        want = F.fold(d.view(c.N, To, c.C * c.ks).transpose(1, 2), (c.T, 1), (c.ks, 1), padding=(c.pad, 0), stride=(c.stride, 1))
        ref = R.reference(c)['dx']
        _close(ref, want[..., 0].transpose(1, 2), 1e-13)
        # the adjoint identity <im2col x, d> = <x, col2im d>
        x = torch.randn(c.N, c.T, c.C, dtype=F64, generator=torch.Generator().manual_seed(5))
        lhs = (R.im2col_ref(c, {'x': x})['col'] * d).sum()
        assert abs(lhs - (x * ref).sum()) <= 1e-12 * (1 + abs(lhs))
        unread = sorted(set(range(c.T)) - set(R.tap_frames(c)[0][R.tap_frames(c)[1]].tolist()))
        assert bool((ref[:, unread] == 0).all())
    assert any('frames no window reads: [2, 5, 8]' in c.reach for c in R.COL2IM) and any('[8]' in c.reach for c in R.COL2IM)
    for c in R.DW_FWD:
        i = R.make_inputs(c.name)
        x, w = i['x'].double().requires_grad_(), i['w'].double().requires_grad_()
        b = torch.zeros(c.C, dtype=F64, requires_grad=True) if i['b'] is None else i['b'].double().requires_grad_()
        y = F.conv1d(x.transpose(1, 2), w[:, None], b, c.stride, c.pad, groups=c.C).transpose(1, 2)
        _close(R.reference(c)['y'], y.detach(), 1e-13)
        y.backward(i['dy'].double())
        cb = R.BY_NAME[c.name.replace('dw_fwd', 'dw_bwd')]
        ref = R.reference(cb)
        ib = R.make_inputs(cb.name)
        xb, wb = ib['x'].double().requires_grad_(), ib['w'].double().requires_grad_()
        bb = torch.zeros(c.C, dtype=F64, requires_grad=True)
        F.conv1d(xb.transpose(1, 2), wb[:, None], bb, c.stride, c.pad, groups=c.C).transpose(1, 2).backward(ib['dy'].double())
        _close(ref['dw'], wb.grad, 1e-12)
        assert ('dx' in ref) == cb.want_dx and ('db' in ref) == cb.has_bias
        if cb.want_dx:
            _close(ref['dx'], xb.grad, 1e-13)
        if cb.has_bias:
            _close(ref['db'], bb.grad, 1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# exact cases, the rail, the mutants
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in R.ALL_CASES if c.mode == 'exact'])
def test_exact_cases_are_exact(name):
    c = R.BY_NAME[name]
    ref, st = R.reference(c), R.stand_in(c)
    assert ref.keys() == st.keys() and ref
    for k in ref:
        assert st[k].dtype == torch.float32
        assert R.same_bits(st[k], ref[k].float()), (name, k)                  # (no -0.0 against +0.0 either)
        assert len(ref[k].unique()) >= min(3, ref[k].numel()), (name, k, 'degenerate')
        if c.launch not in ('embed_fwd', 'add_rows'):                        # those two round one fp32 add; everything else is representable
            assert torch.equal(st[k].double(), ref[k]), (name, k)
    if name.endswith('_int'):
        for t in R.make_inputs(name).values():
            if t is not None and t.dtype == torch.float32:
                assert bool((t == t.round()).all()) and float(t.abs().max()) <= 2


@pytest.mark.parametrize('name', [c.name for c in R.ALL_CASES if c.mode != 'exact'])
def test_stand_in_is_fp32_noise(name):
    """A rail for the stand-in only: inside 4 x 2^-22 S of the float64 reference on every element of every random case, so that no bound
    grows past 16 x 2^-22."""
    c = R.BY_NAME[name]
    n, b = R.noise(c), R.bound(c)
    print(name, {k: f'{n[k]:.2e} -> {b[k]:.2e}' for k in n})
    ref, S = R.reference(c), R.scale(c)
    assert n.keys() == ref.keys() == S.keys() == R.stand_in(c).keys()
    for k in n:
        assert n[k] <= RAIL, (name, k, n[k])
        assert R.FLOOR <= b[k] <= R.FACTOR * RAIL
        assert bool((S[k] >= 0).all()) and S[k].shape == ref[k].shape


def _caught(c, mutant):
    """How far outside the allowed error the mutant lies, in units of it, over the outputs (exact / standin case: inf when a bit differs)."""
    ref, mut = R.reference(c), R.reference(c, mutant)
    if c.mode == 'exact':
        return float('inf') if any(not torch.equal(mut[k], ref[k]) for k in ref) else 0.0
    S, b = R.scale(c), R.bound(c)
    return max(R.excess(mut[k], ref[k], S[k], b[k]) for k in ref)


@pytest.mark.parametrize('launch', list(R.MUTANTS))
def test_every_mutant_is_caught_on_every_case_it_applies_to(launch):
    for mutant, (what, _) in R.MUTANTS[launch].items():
        cases = [c for c in R.FAMILIES[launch] if R.mutant_applies(mutant, c)]
        assert cases, (mutant, 'no case')
        if any(c.mode == 'exact' for c in R.FAMILIES[launch]):
            assert any(c.mode == 'exact' for c in cases), (mutant, 'needs an exact case')
        worst = {}
        for c in cases:
            worst[c.name] = e = _caught(c, mutant)
            assert e >= 2.0, (mutant, what, c.name, e)
            if c.mode == 'standin':
                assert any(not torch.equal(R.reference(c, mutant)[k].float(), R.stand_in(c)[k]) for k in R.stand_in(c))
        finite = [e for e in worst.values() if e != float('inf')]
        print(f'{launch} {mutant}: {len(cases)} cases' + (f', outside by {min(finite):.3g} .. {max(finite):.3g} x the allowed error' if finite else ''))
    for c in R.FAMILIES[launch]:                                             # a mutant that does not apply leaves the case alone
        for mutant in R.MUTANTS[launch]:
            if not R.mutant_applies(mutant, c) and (launch, mutant) not in R.NUMERIC_ONLY:
                ref, mut = R.reference(c), R.reference(c, mutant)
                assert all(torch.equal(mut[k], ref[k]) for k in ref), (mutant, c.name)


# ------------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_reach_every_edge():
    ln = R.LN_FWD
    assert {c.C for c in ln} == {1, 3, 63, 64, 65, 200, 768, 1028} and {c.rows for c in ln} == {1, 5, 37}
    assert {(c.bias, c.dist) for c in ln} == {(True, 'wide'), (True, 'far'), (False, 'wide'), (False, 'far')}
    for c in ln:
        x = R.make_inputs(c.name)['x']
        assert c.rows < 5 or bool((x[3] == x[3, 0]).all())
    lb = R.LN_BWD
    assert {c.C for c in lb} >= {4, 252, 256, 260, 1024, 1028, 2048, 2052, 201} and {c.rows for c in lb if c.C == 8} == {1, 3, 5, 2049, 2053}
    assert {R.ln_bwd_path(c) for c in lb if c.C in (2052, 201) or c.offset} == {'twopass'}
    assert {R.ln_bwd_path(c) for c in lb if c.C not in (2052, 201) and not c.offset} == {'fused'}
    assert {c.C for c in lb if c.bf16} == {256, 1028} and {c.dres for c in lb} == {True, False} and {c.has_bias for c in lb} == {True, False}
    ce = R.CE
    assert {c.V for c in ce if c.ld == c.V and not c.offset} == {1, 3, 4, 333, 1024, 1028, 5000, 2048}
    assert {(c.V, c.ld) for c in ce if c.ld != c.V} == {(1030, 1032), (1024, 1025)} and sum(c.offset for c in ce) == 1
    assert {c.ignore for c in ce} == {0, -100} and {c.scale for c in ce} == {1.0, 30.0} and {c.grad1 for c in ce} == {True, False}
    assert all(c.rows == 9 for c in ce) and {c.ninf for c in ce} == {None, 'scattered', 'half'}
    assert {(c.vec, c.V % 4 != 0) for c in ce} >= {(True, False), (True, True), (False, False), (False, True)}
    half = R.make_inputs('ce-V2048_ign-100_s1_half')
    assert bool(torch.isinf(half['x'][:, :1024]).all()) and int(half['tgt'][half['tgt'] != -100].min()) >= 1024
    for c in ce:
        i = R.make_inputs(c.name)
        assert int(i['tgt'][5]) == c.V - 1 and (c.ignore == 0 or int(i['tgt'][0]) in (0, 1024))
        assert len(i['x'][2][torch.isfinite(i['x'][2])].unique()) == 1
        fin = torch.where(torch.isinf(i['x'][1]), torch.full_like(i['x'][1], -1e30), i['x'][1]).sort().values
        assert c.V == 1 or fin[-1] - fin[-2] >= 79
    lsm = R.LSM_FWD
    assert {c.cols for c in lsm} == {1, 29, 64, 65, 1000} and {c.rows for c in lsm} == {1, 6} and {c.scale for c in lsm} == {1.0, 30.0}
    assert any(c.ninf for c in lsm) and [c.tag for c in lsm] == [c.tag for c in R.LSM_BWD]
    assert {c.rows for c in R.COLSUM} == {1, 31, 32, 33, 127, 128, 129, 300} and {c.cols for c in R.COLSUM} == {1, 31, 33, 200}
    for cases in (R.GELU_FWD, R.GELU_BWD):
        assert {(c.kind, c.n) for c in cases} == {(k, n) for k in ('tanh', 'erf') for n in (1, 255, 257)}
    ef = R.EMBED_FWD
    assert {c.C for c in ef} == {4, 100, 300} and {c.B * c.T for c in ef} == {1, 21} and {c.pos0 for c in ef if c.wpe} == {0, 5}
    assert {c.wpe for c in ef} == {True, False}
    eb = R.EMBED_BWD
    assert {(c.wte, c.wpe) for c in eb} == {(True, True), (True, False), (False, True)} and {c.acc for c in eb if c.wpe} == {True, False}
    assert {c.ids for c in eb} == {'same', 'mixed'} and any(c.pos0 == 5 for c in eb) and {c.mode for c in eb} == {'bound', 'exact'}
    assert {c.mode for c in R.EMBED_ORD} == {'standin', 'exact'} and any(c.C > 256 for c in R.EMBED_ORD)
    geos = {(c.ks, c.stride, c.pad, c.T) for c in R.IM2COL}
    assert geos == {(3, 2, 1, 1), (3, 2, 1, 2), (3, 2, 1, 7), (3, 2, 1, 8), (3, 1, 1, 5), (5, 4, 3, 43), (2, 3, 0, 11), (1, 1, 0, 4), (4, 2, 0, 9)}
    assert geos == {(c.ks, c.stride, c.pad, c.T) for c in R.COL2IM if c.mode == 'bound'}
    assert {c.N for c in R.IM2COL} == {1, 3} and {c.C for c in R.IM2COL} == {1, 3, 80} and any(c.mode == 'exact' for c in R.COL2IM)
    dw = R.DW_BWD
    assert {c.C for c in dw} == {1, 48, 300} and {c.ks for c in dw} == {1, 3, 8} and {c.rows for c in dw} >= {1, 63, 64, 65, 200}
    assert {(c.stride, c.pad) for c in dw} <= {(2, 1), (1, 1), (4, 3), (3, 0), (1, 0), (2, 0)}
    assert any(c.rows == 65 and c.used == 33 for c in dw) and {c.want_dx for c in dw} == {True, False} and {c.has_bias for c in dw} == {True, False}
    assert any(not c.bias for c in R.DW_FWD)
    for c in R.ALL_CASES:                                                    # no case larger than 2053 x 8 or 9 x 5000
        for t in R.make_inputs(c.name).values():
            assert t is None or t.numel() <= 9 * 5000


def test_every_table_entry_is_consumed_by_the_gpu_file():
    import test_gpu_rows_f64 as G
    assert set(G.RUNNERS) == set(R.FAMILIES)
    assert [c.name for c in G.CASES] == IDS and len(set(IDS)) == len(IDS)
    assert G.R is R
