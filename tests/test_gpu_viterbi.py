"""GPU checks of forced alignment (csrc/viterbi.hip: haloop_amd.ctc.ctc_viterbi, haloop_amd.transducer.transducer_viterbi /
transducer_align, and the two heads' ``align``) against the float64 yardstick tests/viterbi_ref.py on the same fp32 inputs
(tests/test_viterbi_cpu.py validates the yardstick by enumeration and proves the fixtures' gap condition).

On every compared row (all but those ``viterbi_ref.LEFT_OUT`` names) alignments, starts, ends and frames are exact, and a score is
within (terms) * 2^-23 * |score_ref|: a path's score is a sum of `terms` fp32 log-probabilities taken in path order, each addition
rounding by at most 2^-24 of a partial sum that |score| bounds.  terms = T for a CTC path (one emission per frame) and T + U for a
transducer path (T blanks and U labels).  Every figure is printed before it is asserted."""
import math

import pytest
import torch

import viterbi_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -23


def run_ctc(lp, targets, il, tl):
    from haloop_amd import ctc
    return tuple(x.cpu() for x in ctc.ctc_viterbi(lp, targets.to(DEV), None if il is None else il.to(DEV), tl.to(DEV)))


def check_ctc(name, out, rows, il, tl, compared, T):
    scores, ali, starts, ends = out
    worst = 0.0
    for n in compared:
        r, i, u = rows[n], int(il[n]), int(tl[n])
        assert (ali[n, i:] == -1).all() and (starts[n, u:] == -1).all() and (ends[n, u:] == -1).all(), (name, n)
        if r['alignment'] is None:
            assert float(scores[n]) == -math.inf, (name, n)
            assert (ali[n] == -1).all() and (starts[n] == -1).all() and (ends[n] == -1).all(), (name, n)
            continue
        assert ali[n, :i].tolist() == r['alignment'], (name, n)
        assert starts[n, :u].tolist() == r['starts'] and ends[n, :u].tolist() == r['ends'], (name, n)
        err, tol = abs(float(scores[n]) - r['score']), T * EPS * abs(r['score'])
        worst = max(worst, err / tol if tol else err)
        assert err <= tol, (name, n, err, tol)
    print(f'{name}: {len(compared)} rows compared, worst score error {worst:.3f} of its tolerance')


@pytest.mark.parametrize('name', sorted(R.CTC_FIXTURES))
def test_ctc_fixture(name):
    lp, targets, il, tl, rows = R.ctc_fixture(name)
    out = run_ctc(lp.to(DEV), targets, il, tl)
    check_ctc(name, out, rows, il, tl, R.compared_rows('ctc', name), lp.shape[0])


def test_ctc_strided_view_gives_the_same_bits():
    lp, targets, il, tl, rows = R.ctc_fixture('bench')
    a = run_ctc(lp.to(DEV), targets, il, tl)
    ntc = lp.to(DEV).permute(1, 0, 2).contiguous()                              # [N, T, C] memory, read as [T, N, C]
    view = ntc.permute(1, 0, 2)
    assert not view.is_contiguous()
    b = run_ctc(view, targets, il, tl)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    check_ctc('bench (strided)', b, rows, il, tl, R.compared_rows('ctc', 'bench'), lp.shape[0])


def test_ctc_empty_rows_and_cpu_tensors():
    from haloop_amd import _lib, ctc
    lp, targets, il, tl = R.ctc_inputs('bench')
    N, T = lp.shape[1], lp.shape[0]
    il0 = torch.zeros(N, dtype=torch.long)
    tl0 = torch.zeros(N, dtype=torch.long)
    tl0[1::2] = 1
    scores, ali, starts, ends = run_ctc(lp.to(DEV), targets, il0, tl0)            # no frames: score 0 for an empty target, else infeasible
    assert scores[0::2].tolist() == [0.0] * len(scores[0::2]) and (scores[1::2] == -math.inf).all()
    assert (ali == -1).all() and (starts == -1).all() and (ends == -1).all()
    scores, ali, starts, ends = run_ctc(lp.to(DEV), targets, None, tl0 * 0)   # no lengths: every frame
    want = lp[:, :, 0].double().sum(0)                                           # the all-blank path
    assert (ali == 0).all() and (starts == -1).all()
    assert ((scores.double() - want).abs() <= T * EPS * want.abs()).all()
    with pytest.raises(_lib.HaloError):
        ctc.ctc_viterbi(lp, targets, il, tl)


def run_transducer(route, f, g, joint, targets, tn, un):
    from haloop_amd import transducer
    if route == 'dense':
        out = transducer.transducer_viterbi(joint.to(DEV), targets.to(DEV), tn.to(DEV), un.to(DEV))
    else:
        out = transducer.transducer_align(f.to(DEV), g.to(DEV), targets.to(DEV), tn.to(DEV), un.to(DEV))
    return tuple(x.cpu() for x in out)


def check_transducer(name, out, rows, un, compared, terms):
    scores, frames = out
    worst = 0.0
    for n in compared:
        r, u = rows[n], int(un[n])
        assert (frames[n, u:] == -1).all(), (name, n)
        if r['frames'] is None:
            assert float(scores[n]) == -math.inf and (frames[n] == -1).all(), (name, n)
            continue
        assert frames[n, :u].tolist() == r['frames'], (name, n)
        err, tol = abs(float(scores[n]) - r['score']), terms * EPS * abs(r['score'])
        worst = max(worst, err / tol)
        assert err <= tol, (name, n, err, tol)
    print(f'{name}: {len(compared)} rows compared, worst score error {worst:.3f} of its tolerance')


@pytest.mark.parametrize('name', sorted(R.TRANSDUCER_FIXTURES))
def test_transducer_fixture_on_both_routes(name):
    f, g, joint, targets, tn, un, rows = R.transducer_fixture(name)
    compared = R.compared_rows('transducer', name)
    terms = joint.shape[1] + joint.shape[2] - 1
    dense = run_transducer('dense', f, g, joint, targets, tn, un)
    check_transducer(name + ' (dense)', dense, rows, un, compared, terms)
    factors = run_transducer('factors', f, g, joint, targets, tn, un)
    check_transducer(name + ' (factors)', factors, rows, un, compared, terms)
    assert torch.equal(dense[1][compared], factors[1][compared])                # exactly the frames of the dense route


@pytest.mark.parametrize('name', sorted(R.CTC_EXACT))
def test_ctc_wide_lattices_without_rounding(name):
    """More than 512 states: 4, 8, 16 and 30 states per thread, the last at the bound.  Every sum is exact in fp32, so every row equals the
    reference, scores to the bit and ties by the rule."""
    lp, targets, il, tl, rows = R.ctc_exact_fixture(name)
    scores, ali, starts, ends = run_ctc(lp.to(DEV), targets, il, tl)
    for n, r in enumerate(rows):
        i, u = int(il[n]), int(tl[n])
        assert float(scores[n]) == r['score'], (name, n, float(scores[n]), r['score'])
        assert ali[n, :i].tolist() == r['alignment'] and (ali[n, i:] == -1).all(), (name, n)
        assert starts[n, :u].tolist() == r['starts'] and ends[n, :u].tolist() == r['ends'], (name, n)
        assert (starts[n, u:] == -1).all() and (ends[n, u:] == -1).all(), (name, n)


@pytest.mark.parametrize('name', sorted(R.TRANSDUCER_EXACT))
def test_transducer_wide_lattices_without_rounding(name):
    joint, targets, tn, un, rows = R.transducer_exact_fixture(name)
    scores, frames = run_transducer('dense', None, None, joint, targets, tn, un)
    for n, r in enumerate(rows):
        u = int(un[n])
        assert float(scores[n]) == r['score'], (name, n, float(scores[n]), r['score'])
        assert frames[n, :u].tolist() == r['frames'] and (frames[n, u:] == -1).all(), (name, n)


def test_tie_rules_on_the_device():
    from haloop_amd import ctc, transducer
    c = R.TIE_CTC
    lp = torch.full((c['T'], 1, c['C']), -2.0, device=DEV)
    scores, ali, starts, ends = ctc.ctc_viterbi(lp, torch.tensor([c['target']], device=DEV), torch.tensor([c['T']], device=DEV),
                                                torch.tensor([len(c['target'])], device=DEV))
    assert scores.tolist() == [-14.0]
    assert ali.tolist() == [[1, 0, 1, 2, 0, 0, 0]]
    assert starts.tolist() == [[0, 2, 3]] and ends.tolist() == [[0, 2, 3]]
    c = R.TIE_TRANSDUCER
    joint = torch.full((1, c['T'], c['U'] + 1, c['K']), -2.0, device=DEV)
    scores, frames = transducer.transducer_viterbi(joint, torch.tensor([c['target']], device=DEV), torch.tensor([c['T']], device=DEV),
                                                   torch.tensor([c['U']], device=DEV))
    assert scores.tolist() == [-12.0]
    assert frames.tolist() == [[0, 0]]


def test_ctc_score_is_one_term_of_the_forward_sum():
    from haloop_amd import ops
    for name in ('bench', 'small_vocab'):
        lp, targets, il, tl = R.ctc_inputs(name)
        d = lp.to(DEV)
        tg = targets.clamp(max=lp.shape[2] - 1).to(DEV)                           # the padding as labels the alpha kernel may touch
        scores = ops.ctc_viterbi(d, True, tg, il.to(DEV), tl.to(DEV))[0].cpu()
        nll = ops.ctc_fwd(d, True, tg, il.to(DEV), tl.to(DEV))[0].cpu()
        print(f'{name}: max (viterbi score + nll) = {float((scores + nll).nan_to_num(neginf=-1.0, nan=-1.0).max()):.3e}')
        for n in range(lp.shape[1]):
            if float(nll[n]) == math.inf:
                assert float(scores[n]) == -math.inf
            else:
                assert float(scores[n]) <= -float(nll[n]) + 1e-5 * abs(float(nll[n]))


def test_ctc_alignment_of_the_greedy_hypothesis_is_the_greedy_alignment():
    from haloop_amd import ctc, ops
    lp = R.ctc_inputs('bench')[0].to(DEV)
    T, N, _ = lp.shape
    greedy, _, hyp, hyp_len = ops.ctc_greedy(lp.permute(1, 0, 2).contiguous())
    S = int(hyp_len.max())
    assert S >= 1
    scores, ali, starts, ends = ctc.ctc_viterbi(lp, hyp[:, :S], torch.full((N,), T, device=DEV), hyp_len)
    assert torch.equal(ali, greedy)                                             # the best labelling overall is the best of its own collapse
    assert (scores > -math.inf).all()


def test_transducer_score_is_one_term_of_the_forward_sum():
    from haloop_amd import transducer
    f, g, joint, targets, tn, un = R.transducer_inputs('bench')
    scores, _ = run_transducer('dense', f, g, joint, targets, tn, un)
    losses = transducer.transducer_forward_score(joint.to(DEV), targets.to(DEV), tn.to(DEV), un.to(DEV)).cpu()
    print(f'max (viterbi score + loss) = {float((scores + losses).max()):.3e}')
    assert (scores <= -losses + 1e-5 * losses.abs()).all()


def _head_inputs(N=4, T=12, U=3, V=9):
    gen = torch.Generator().manual_seed(5)
    features = torch.randn(N, T, 32, generator=gen) * 4
    targets = torch.randint(1, V, (N, U), generator=gen)
    return features, targets, torch.tensor([12, 10, 12, 7]), torch.tensor([3, 2, 3, 1])


def test_temporal_classifier_align():
    from haloop_amd import _lib, ctc, recognizer
    torch.manual_seed(11)
    head = recognizer.TemporalClassifier(32, 9).to(DEV).eval()
    features, targets, il, tl = _head_inputs()
    got = head.align(features.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV))
    lp = head.log_probs(features.to(DEV)).detach().permute(1, 0, 2)              # the head's own device log-probabilities
    want = ctc.ctc_viterbi(lp, targets.to(DEV), il.to(DEV), tl.to(DEV))
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    rows = R.ctc_align(lp.cpu(), targets, il, tl)
    compared = [n for n, r in enumerate(rows) if r['gap'] >= R.GAP]
    print('TemporalClassifier.align: gaps', [f"{r['gap']:.3g}" for r in rows])
    assert 2 * len(compared) >= len(rows)
    check_ctc('TemporalClassifier.align', tuple(x.cpu() for x in got), rows, il, tl, compared, features.shape[1])
    with pytest.raises(_lib.HaloError):
        head.align(features, targets, il, tl)
    head.train()
    with pytest.raises(NotImplementedError):
        head.align(features.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV))


def test_transducer_head_align():
    from haloop_amd import _lib, functional as HF, recognizer, transducer
    torch.manual_seed(12)
    head = recognizer.Transducer(32, 9).to(DEV).eval()
    features, targets, il, tl = _head_inputs()
    N = features.shape[0]
    got = head.align(features.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV))
    with torch.no_grad():                                                        # the head's own device factors, as forward builds them
        lm_targets = torch.cat([targets.new_zeros((N, 1)), targets], dim=1).to(DEV)
        g, _ = head.lm.forward_batch_first(lm_targets, head.lm.init_hidden(N))
        f = HF.linear(features.to(DEV), head.classifier.weight, head.classifier.bias)
    want = transducer.transducer_align(f, g, targets.to(DEV), il.to(DEV), tl.to(DEV))
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    joint = (f[:, :, None, :] + g[:, None, :, :]).log_softmax(-1).cpu()
    rows = R.transducer_align(joint, targets, il, tl)
    compared = [n for n, r in enumerate(rows) if r['gap'] >= R.GAP]
    print('Transducer.align: gaps', [f"{r['gap']:.3g}" for r in rows])
    assert 2 * len(compared) >= len(rows)
    check_transducer('Transducer.align', tuple(x.cpu() for x in got), rows, tl, compared, joint.shape[1] + joint.shape[2] - 1)
    with pytest.raises(_lib.HaloError):
        head.align(features, targets, il, tl)
    with pytest.raises(NotImplementedError):
        head.align(features.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV), prompt=targets)
    head.train()
    with pytest.raises(NotImplementedError):
        head.align(features.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV))


def test_two_runs_give_the_same_bits():
    lp, targets, il, tl = R.ctc_inputs('two_waves')
    d = lp.to(DEV)
    for x, y in zip(run_ctc(d, targets, il, tl), run_ctc(d, targets, il, tl)):
        assert torch.equal(x, y)
    args = R.transducer_inputs('bench')
    for route in ('dense', 'factors'):
        for x, y in zip(run_transducer(route, *args), run_transducer(route, *args)):
            assert torch.equal(x, y)
