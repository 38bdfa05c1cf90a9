"""Float64 restatement, on the CPU in plain torch, of greedy RNN-transducer search ([Graves12]) for haloop_amd.recognizer.Transducer,
and the fixtures that tests/test_rnnt_greedy_cpu.py and tests/test_gpu_rnnt_decode.py share.  No tests in here.

The modules are built from a ``Transducer`` state dict by the name map of tests/test_gpu_lattice.py:153-162: ``lm.rnn.*`` ->
``torch.nn.LSTM(512, 512, 2)``, ``lm.embedding.weight`` -> the embedding and (tied) the ``out_layer`` weight, ``lm.out_layer.bias``,
``classifier.*``.  With F = classifier(features) the search of row n is

    state = zeros; g = out_layer(lstm_step(embedding[0], state))        # the zero prefix of training
    t = u = here = 0; score = 0
    while t < input_lengths[n] and u < capacity:
        lp = log_softmax(F[n, t] + g)
        k = 0 if here == max_symbols_per_frame else argmax(lp)           # lowest index among equal maxima
        score += lp[k]
        if k == 0: t += 1; here = 0
        else:      tokens[u] = k; frames[u] = t; u += 1; here += 1; g = out_layer(lstm_step(embedding[k], state))

A row that ends with u == capacity is truncated; input_lengths are clipped to T; frames at or past a row's length are never read.
"""
import functools

import torch

E = 512          # emb_dim == hidden_dim of the arch's prediction network (ha/init.py:180-185)
LAYERS = 2


def modules(sd):
    """-> (lstm, embedding [V, E], out_bias [V], classifier weight [V, feat], classifier bias [V]), all float64."""
    lstm = torch.nn.LSTM(E, E, LAYERS).double()
    lstm.load_state_dict({k[len('lm.rnn.'):]: v.double() for k, v in sd.items() if k.startswith('lm.rnn.')})
    return (lstm, sd['lm.embedding.weight'].double(), sd['lm.out_layer.bias'].double(), sd['classifier.weight'].double(),
            sd['classifier.bias'].double())


@torch.no_grad()
def greedy(sd, features, input_lengths, capacity, max_symbols_per_frame=10):
    """-> dict(tokens [N, capacity] int64 (-1 past the length), lengths [N], frames [N, capacity] (-1 past the length), scores [N]
    float64, truncated [N] bool, forced [N] int64: forced blanks taken, gap: the smallest difference between the two largest entries of
    lp over every visited node whose argmax was free (inf when there was none))."""
    lstm, emb, ob, cw, cb = modules(sd)
    N, T, _ = features.shape
    F = torch.nn.functional.linear(features.double(), cw, cb)
    tokens, frames = torch.full((N, capacity), -1, dtype=torch.int64), torch.full((N, capacity), -1, dtype=torch.int64)
    lengths, forced = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    scores, truncated = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.bool)
    gap = float('inf')
    for n in range(N):
        L = max(0, min(int(input_lengths[n]), T))
        state = (torch.zeros(LAYERS, 1, E, dtype=torch.float64), torch.zeros(LAYERS, 1, E, dtype=torch.float64))

        def step(k, state):
            out, state = lstm(emb[k].view(1, 1, E), state)
            return torch.nn.functional.linear(out.view(E), emb, ob), state
        g, state = step(0, state)
        t = u = here = 0
        while t < L and u < capacity:
            lp = (F[n, t] + g).log_softmax(-1)
            if here == max_symbols_per_frame:
                k = 0
                forced[n] += 1
            else:
                k = int((lp == lp.max()).nonzero()[0])
                top = lp.topk(2).values
                gap = min(gap, float(top[0] - top[1]))
            scores[n] += lp[k]
            if k == 0:
                t, here = t + 1, 0
            else:
                tokens[n, u], frames[n, u] = k, t
                u, here = u + 1, here + 1
                g, state = step(k, state)
        lengths[n] = u
        truncated[n] = u == capacity
    return dict(tokens=tokens, lengths=lengths, frames=frames, scores=scores, truncated=truncated, forced=forced, gap=gap)


@torch.no_grad()
def teacher_forced_joint(sd, features_row, hyp):
    """log_softmax joint [T, U + 1, V] (float64) of one row: nn.LSTM teacher-forced on [0 | hyp], the additive joint of training."""
    lstm, emb, ob, cw, cb = modules(sd)
    lm_in = torch.cat([hyp.new_zeros(1), hyp])
    out, _ = lstm(emb[lm_in].view(-1, 1, E))
    lm_out = torch.nn.functional.linear(out.view(-1, E), emb, ob)                    # [U + 1, V]
    f = torch.nn.functional.linear(features_row.double(), cw, cb)                   # [T, V]
    return (f[:, None, :] + lm_out[None, :, :]).log_softmax(-1)


# ---- fixtures: a random-initialised Transducer whose blank bias is raised (classifier.bias[0] += 2.0) under a cap of two symbols per
#      frame; without the cap an untrained model emits to capacity at frame 0 or never emits.  The seeds were searched on the CPU with
#      this file's loop for the conditions tests/test_rnnt_greedy_cpu.py asserts. ----
MAX_SYMBOLS = 2
SMALL_SEED, ROWS17_SEED = 31, 1
FIXTURES = {
    # name: (seed, N, T, feat, V, input_lengths (None: drawn from the seed, one 0 among them), capacity)
    'small': dict(seed=SMALL_SEED, N=3, T=12, feat=48, V=20, lengths=[12, 9, 1], capacity=6),
    'rows17': dict(seed=ROWS17_SEED, N=17, T=23, feat=64, V=67, lengths=None, capacity=10),
    'rows17_long': dict(seed=ROWS17_SEED, N=17, T=23, feat=64, V=67, lengths=None, capacity=46),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (state dict (float32, CPU), features [N, T, feat] float32, input_lengths [N] int64, capacity, reference dict).  Computed once
    per process; callers must not modify what they get."""
    from haloop_amd import recognizer
    f = FIXTURES[name]
    gen = torch.Generator().manual_seed(f['seed'])
    saved = torch.get_rng_state()
    torch.manual_seed(f['seed'])
    head = recognizer.Transducer(f['feat'], f['V']).eval()
    torch.set_rng_state(saved)
    sd = {k: v.detach().clone() for k, v in head.state_dict().items()}
    sd['classifier.bias'][0] += 2.0
    features = torch.randn(f['N'], f['T'], f['feat'], generator=gen)
    if f['lengths'] is None:
        il = torch.randint(1, f['T'] + 1, (f['N'],), generator=gen)
        il[int(torch.randint(0, f['N'], (1,), generator=gen))] = 0
    else:
        il = torch.tensor(f['lengths'])
    return sd, features, il, f['capacity'], greedy(sd, features, il, f['capacity'], MAX_SYMBOLS)
