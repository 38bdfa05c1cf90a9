"""GPU checks of the launch sequences of the five beam searches that carry an ``rnn.Decoder`` across their slots
(``transducer.BeamDecoder`` / ``BeamStream``, ``fusion.CTCFusionDecoder`` / ``TransducerFusionDecoder`` / ``AttentionFusionDecoder``), as
their class docstrings state them.

The public ``ops`` launch wrappers are wrapped and every call of one decode is recorded with its tensors' addresses.  Asserted:

    the whole sequence of names, prologue included (the network after its start token: ``L`` cells and one ``decode_linear``);
    the parity copies: a step reads h, c and g where the cells (and the keep) of the step before wrote them, and the two copies alternate;
    a second decode on the same object passes the addresses of the first: nothing is allocated per call.

Shapes: the smallest the fused rule admits (H = E = 512), V = 32, N = 2, W = 3, T = 6, capacity = 4; the first network has two layers and
the LM one, so a depth taken from the wrong network shows.  The attention decoder is 768 wide, so that the LM's ``decode_linear`` (K = 512)
is told from the decoder's own.
"""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H, V, N, W, T, CAP = 512, 32, 2, 3, 6, 4
STEPS = ('rnnt_beam_step', 'rnnt_beam_step_stream', 'ctc_lm_beam_step', 'rnnt_lm_beam_step', 'decode_beam_select_lm')
INPUTS = ('f', 'input_lengths', 'emissions', 'emission_lengths')      # the call's own tensors: not the decoder's buffers
WRAPPED = STEPS + ('rnnt_beam_stream_open', 'rnnt_lstm_cell', 'decode_linear', 'rnnt_beam_keep')


@pytest.fixture(scope='module')
def hal():
    from haloop_amd import _lib, fusion, ops, recognizer, rnn, transducer, transformer
    _lib.lib()
    _lib.lend_scratch()
    prev = _lib.get_math_mode()
    _lib.set_math_mode('bf16x3')
    yield dict(ops=ops, lib=_lib, fusion=fusion, rec=recognizer, rnn=rnn, td=transducer, tr=transformer)
    _lib.set_math_mode(prev)


@pytest.fixture
def calls(hal, monkeypatch):
    """The recorded launches: (name, {argument name: address of a tensor, None, or the tensor's shape under 'shape:' + name})."""
    out = []

    def wrap(name):
        real = getattr(hal['ops'], name)
        sig = inspect.signature(real)

        def recorded(*a, **k):
            args = sig.bind(*a, **k).arguments
            entry = {n: v.data_ptr() for n, v in args.items() if torch.is_tensor(v)}
            entry.update({'shape:' + n: tuple(v.shape) for n, v in args.items() if torch.is_tensor(v)})
            out.append((name, entry))
            return real(*a, **k)
        monkeypatch.setattr(hal['ops'], name, recorded)
    for name in WRAPPED:
        wrap(name)
    return out


def _head(hal, seed=1):
    torch.manual_seed(seed)
    head = hal['rec'].Transducer(16, V)                                     # its prediction network: E = H = 512, two layers
    assert head.lm.num_layers == 2 and head.lm.hidden_dim == H
    return head.to(DEV).eval()


def _lm(hal, seed=2):
    torch.manual_seed(seed)
    return hal['rnn'].Decoder(V, H, H, 1).to(DEV).eval()


def _features(C=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, T, C, generator=g).to(DEV), torch.tensor([T, T - 2], device=DEV)


def _network(step, prefix=''):
    """(g, h_in, c_in, c_out) of one network in a recorded step: the addresses the step reads and the c copy it gathers into."""
    g = step['lm_logits'] if 'lm_logits' in step else step[('lg' if prefix else 'g')]
    x = prefix if 'lm_logits' not in step else ''
    return g, step.get(x + 'h_in'), step.get(x + 'c_in'), step.get(x + 'c_out')


def _cells(group):
    """(h, c, g) the cells of one recorded group wrote: layer 0's h_next and c are the bases of their copies."""
    return group[0][1]['h_next'], group[0][1]['c'], group[-1][1]['out']


def _split(record, layers, keep):
    """The record of one network as (prologue cells, [(step, cells or None, keep or None)]): asserts the order on the way.  ``layers``:
    per network; every step but the last is followed, per network, by its cells, one linear and (``keep``) one keep."""
    names = [n for n, _ in record]
    pro = sum(layers) + len(layers)
    want = [x for L in layers for x in ['rnnt_lstm_cell'] * L + ['decode_linear']]
    after = [x for L in layers for x in ['rnnt_lstm_cell'] * L + ['decode_linear'] + (['rnnt_beam_keep'] if keep else [])]
    assert names[:pro] == want, names[:pro]
    rest, rounds, i = record[pro:], [], 0
    while i < len(rest):
        assert rest[i][0] in STEPS, (i, rest[i][0])
        chunk = rest[i + 1:i + 1 + len(after)]
        if i + 1 == len(rest):
            rounds.append((rest[i][1], None))                               # the last step runs alone
            break
        assert [n for n, _ in chunk] == after, (i, [n for n, _ in chunk])
        rounds.append((rest[i][1], chunk))
        i += 1 + len(after)
    prologue, at = [], 0
    for L in layers:
        prologue.append(record[at:at + L + 1])
        at += L + 1
    return prologue, rounds


def _assert_parity(prologue, rounds, layers, keep, copies=2):
    """Every step reads what the launches before it wrote; the copies alternate (``copies`` = 1: g has one copy, as on the attention side)."""
    per = [L + 1 + (1 if keep else 0) for L in layers]
    for x, L in enumerate(layers):
        prefix = 'lm_' if x else ''
        written = _cells(prologue[x])
        for i, (step, chunk) in enumerate(rounds):
            g, h_in, c_in, c_out = _network(step, prefix)
            if h_in is None:                                                # the attention side's last step gathers nothing
                assert chunk is None and g == written[2]
                continue
            assert (h_in, c_in, g) == written, (x, i)
            if chunk is None:
                continue
            at = sum(per[:x])
            group = chunk[at:at + per[x]]
            written = _cells(group[:L + 1])
            assert written[1] == c_out and written[0] != h_in and written[1] != c_in, (x, i)
            assert (written[2] != g) == (copies == 2), (x, i)
            assert all(e['shape:c'][0] == N * W for _, e in group[:L]), (x, i)
            if keep:
                k = group[-1][1]
                assert (k['h_in'], k['c_in'], k['g_in'], k['h_out'], k['c_out'], k['g_out']) == (h_in, c_in, g) + written, (x, i)
        steps = [_network(s, prefix)[1] for s, _ in rounds if _network(s, prefix)[1] is not None]
        assert all(a != b for a, b in zip(steps, steps[1:])) and all(a == b for a, b in zip(steps, steps[2:])), x


def _twice(calls, decode):
    """The records of two decodes on one object: the second passes the addresses of the first."""
    decode()
    first = list(calls)
    del calls[:]
    decode()
    held = lambda record: [(n, {k: v for k, v in e.items() if k not in INPUTS}) for n, e in record]
    assert held(first) == held(calls)
    return first


def test_beam_decoder(hal, calls):
    head = _head(hal)
    dec = hal['td'].BeamDecoder(head, N, CAP, W)
    assert dec.fused
    x, il = _features()
    record = _twice(calls, lambda: dec.decode(x, il))
    prologue, rounds = _split(record, [2], keep=True)
    assert len(rounds) == dec.iterations and all(s['shape:h_in'] == (2, N * W, H) for s, _ in rounds)
    _assert_parity(prologue, rounds, [2], keep=True)


def test_ctc_fusion_decoder(hal, calls):
    lm = _lm(hal)
    dec = hal['fusion'].CTCFusionDecoder(lm, N, CAP, W)
    assert dec.fused
    g = torch.Generator().manual_seed(5)
    e = torch.randn(T, N, V, generator=g).log_softmax(-1).to(DEV)
    record = _twice(calls, lambda: dec.decode(e, torch.tensor([T, T - 2], device=DEV)))
    prologue, rounds = _split(record, [1], keep=True)
    assert len(rounds) == dec.iterations == T
    _assert_parity(prologue, rounds, [1], keep=True)


def test_transducer_fusion_decoder(hal, calls):
    head, lm = _head(hal), _lm(hal)
    dec = hal['fusion'].TransducerFusionDecoder(head, lm, N, CAP, W)
    assert dec.fused
    x, il = _features()
    record = _twice(calls, lambda: dec.decode(x, il))
    prologue, rounds = _split(record, [2, 1], keep=True)                    # the prediction network's two layers, then the LM's one
    assert len(rounds) == dec.iterations
    assert all(s['shape:h_in'] == (2, N * W, H) and s['shape:lm_h_in'] == (1, N * W, H) for s, _ in rounds)
    _assert_parity(prologue, rounds, [2, 1], keep=True)


def test_attention_fusion_decoder(hal, calls, monkeypatch):
    monkeypatch.setenv('HALO_DECODE_GRAPH', '0')
    torch.manual_seed(4)
    C = 768
    decoder = hal['tr'].Decoder(vocab=V, head_dim=64, heads=12, p_drop=0.0, layers=1).to(DEV).eval()
    dec = hal['fusion'].AttentionFusionDecoder(decoder, _lm(hal), N, CAP, W)
    assert dec.fused
    x, il = _features(C)
    record = _twice(calls, lambda: dec.decode(x, il))
    # the decoder's own products have K = 768 and more: the LM's launches are the cells and the linear over 512 columns
    record = [(n, e) for n, e in record if n != 'decode_linear' or e['shape:x'][1] == H]
    prologue, rounds = _split(record, [1], keep=False)
    assert len(rounds) == CAP and rounds[-1][1] is None
    _assert_parity(prologue, rounds, [1], keep=False, copies=1)


def test_beam_stream(hal, calls):
    head = _head(hal)
    bs = hal['td'].BeamStream(head, N, CAP, W, max_chunk=3)
    assert bs.fused
    with torch.no_grad():
        x, _ = _features()
        f = torch.nn.functional.linear(x, head.classifier.weight, head.classifier.bias).contiguous()
    L, per = 2, 2 + 1 + 2                                                    # a round: step, two cells, linear, keep
    round_names = ['rnnt_beam_step_stream'] + ['rnnt_lstm_cell'] * L + ['decode_linear', 'rnnt_beam_keep']

    def utterance():
        """Two calls of three frames; -> the records of the two calls, each asserted to be an open and complete rounds."""
        out = []
        for j in range(2):
            del calls[:]
            bs.advance(f[:, 3 * j:3 * j + 3], None, [True] * N if j == 0 else None, [True] * N if j == 1 else None)
            out.append(list(calls))
        return out

    first = utterance()
    # the zero state: the prologue on one slot, once per parameter version, before the first open
    zero, first[0] = first[0][:L + 1], first[0][L + 1:]
    assert [n for n, _ in zero] == ['rnnt_lstm_cell'] * L + ['decode_linear']
    assert all(e['shape:xh'] == (1, 2 * H) and e['shape:c'] == (1, H) for _, e in zero[:L])
    rounds = []
    for record in first:
        names = [n for n, _ in record]
        assert names[0] == 'rnnt_beam_stream_open' and (len(names) - 1) % per == 0 and names[1:] == round_names * ((len(names) - 1) // per)
        rounds += [(record[i][1], record[i + 1:i + per]) for i in range(1, len(record), per)]
    assert (len(first[1]) - 1) // per == bs.rounds
    # the open launch fills the copy the first step reads; from there on the parity is carried, across the call boundary too
    o = first[0][0][1]
    s0 = rounds[0][0]
    assert (o['h'], o['c'], o['g']) == (s0['h_in'], s0['c_in'], s0['g'])
    written = (s0['h_in'], s0['c_in'], s0['g'])
    for i, (step, chunk) in enumerate(rounds):
        assert (step['h_in'], step['c_in'], step['g']) == written, i
        new = _cells(chunk[:L + 1])
        k = chunk[-1][1]
        assert new[1] == step['c_out'] and all(a != b for a, b in zip(new, written)), i
        assert (k['h_in'], k['c_in'], k['g_in'], k['h_out'], k['c_out'], k['g_out']) == written + new, i
        written = new
    o2 = first[1][0][1]
    n0 = (len(first[0]) - 1) // per
    assert (o2['h'], o2['c'], o2['g']) == (rounds[n0][0]['h_in'], rounds[n0][0]['c_in'], rounds[n0][0]['g'])
    # a second utterance on the same object: no prologue (the parameters are as they were) and no address the first did not pass
    second = utterance()
    assert second[0][0][0] == 'rnnt_beam_stream_open'
    addresses = lambda records: {(n, k, v) for r in records for n, e in r for k, v in e.items() if not k.startswith('shape:')
                                 and k not in ('h', 'c', 'g', 'h_in', 'c_in', 'g_in', 'h_out', 'c_out', 'g_out', 'h_next', 'out', 'f')}
    copies = lambda records: {v for r in records for n, e in r for k, v in e.items() if k in ('h_in', 'c_in', 'g', 'c_out', 'h_next', 'out')}
    assert addresses(second) <= addresses(first) and copies(second) == copies(first)
