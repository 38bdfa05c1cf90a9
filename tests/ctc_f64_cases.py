"""The inputs of tests/test_gpu_ctc_f64.py, shared with tests/test_ctc_ref_cpu.py (which holds the yardstick to float64 torch on them).

The CTC shapes are chosen from the dispatch rule of halo_ctc_fwd / halo_ctc_bwd (csrc/ctc.hip), quoted here so that a change of the
rule shows up as a case that no longer reaches its path (``ctc_paths`` restates it and the tests assert each case's expected pair):

    forward   single-wave kernel iff 2S+1 <= 64 and T*C*4 <= 60 KiB                 else ctc_alpha_kernel, block = min(1024, roundup64(2S+3))
    backward  single-wave kernel iff 2S+1 <= 64 and (T*C + T*(2S+1))*4 <= 60 KiB    else ctc_beta_grad_kernel, block = min(1024, roundup64(max(2S+1, C) + 2))

and the head's slicing from head_slices (csrc/head.hip), to which head_train_slices passes the device's CU count: slices double while
slices < 8, (H/32) % (2 slices) == 0 and B * 2 slices <= the device's CU count.
"""
import numpy as np
import torch

WAVE_LDS = 60 * 1024


def ctc_paths(T, C, S):
    """-> ('wave' | 'general', 'wave' | 'general', state-loop trips of the general forward, class-loop trips of the general backward)."""
    S_ = 2 * S + 1
    fwd = 'wave' if S_ <= 64 and T * C * 4 <= WAVE_LDS else 'general'
    bwd = 'wave' if S_ <= 64 and (T * C + T * S_) * 4 <= WAVE_LDS else 'general'
    block = lambda n: min(1024, (n + 2 + 63) // 64 * 64)
    return fwd, bwd, -(-S_ // block(S_)) if fwd == 'general' else 1, -(-C // block(max(S_, C))) if bwd == 'general' else 1


def _no_adjacent_repeats(g, N, S, C):
    tg = torch.randint(1, C, (N, S), generator=g)
    for n in range(N):
        for k in range(1, S):
            while tg[n, k] == tg[n, k - 1]:
                tg[n, k] = int(torch.randint(1, C, (1,), generator=g))
    return tg


def _runs(g, N, S, C):
    """Runs of one to three equal labels, neighbouring runs distinct."""
    tg = torch.zeros(N, S, dtype=torch.int64)
    for n in range(N):
        k, last = 0, 0
        while k < S:
            lab = int(torch.randint(1, C, (1,), generator=g))
            if lab == last:
                continue
            run = int(torch.randint(1, 4, (1,), generator=g))
            tg[n, k:k + run] = lab
            k, last = k + run, lab
    return tg


def _ctc_inputs(T, C, S, il, tl, seed, labels='random', scale=1.0):
    N = len(il)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, T, C, generator=g) * scale
    if labels == 'distinct':
        tg = torch.stack([torch.randperm(C - 1, generator=g)[:S] + 1 for _ in range(N)])
    elif labels == 'no_adjacent_repeats':
        tg = _no_adjacent_repeats(g, N, S, C)
    elif labels == 'runs':
        tg = _runs(g, N, S, C)
    else:
        tg = torch.randint(1, C, (N, S), generator=g)
    w = torch.rand(N, generator=g) + 0.5
    return dict(lp=logits.log_softmax(-1), tg=tg, il=torch.tensor(il), tl=torch.tensor(tl), w=w)       # lp is [N, T, C]


def _classes_two_trips(T, il, tl, seed):
    c = _ctc_inputs(T, 1100, 6, il, tl, seed, labels='no_adjacent_repeats')
    c['tg'][0, :3] = torch.tensor([1099, 1024, 1023])        # classes of the second trip of the 1024-thread class loop, and its edge
    return c


def _repeats():
    c = _ctc_inputs(70, 6, 31, [70, 70, 55], [31, 31, 20], 308, labels='runs')
    rep = int((c['tg'][0, 1:] == c['tg'][0, :-1]).sum())
    c['il'][0] = 31 + rep                                    # exactly tl + repeats frames: one alignment, every blank forced
    assert rep >= 5 and 31 + rep <= 70
    return c


def _corners(N):
    """The corners of tests/test_gpu_parity.py::test_ctc_edge_cases_vs_torch_cpu."""
    g = torch.Generator().manual_seed(309 + N)
    tg = torch.tensor([[1, 2, 3, 4, 5, 6],      # tl = 0: empty target
                       [3, 0, 0, 0, 0, 0],      # one label, one frame
                       [1, 2, 3, 4, 0, 0],      # il == tl: every frame a label
                       [2, 2, 2, 0, 0, 0],      # repeats: needs 2 tl - 1 = 5 frames, has 5
                       [2, 2, 2, 0, 0, 0],      # ... has 4: infeasible
                       [6, 5, 6, 5, 6, 5]])     # the full width S, all frames
    il = torch.tensor([7, 1, 4, 5, 4, 12])
    tl = torch.tensor([0, 1, 4, 3, 3, 6])
    logits = torch.randn(N, 12, 7, generator=g)
    return dict(lp=logits.log_softmax(-1), tg=tg[:N].clone(), il=il[:N].clone(), tl=tl[:N].clone(), w=torch.rand(N, generator=g) + 0.5)


def _masked():
    g = torch.Generator().manual_seed(311)
    logits = torch.randn(3, 12, 6, generator=g)
    logits[:, :, 5] = float('-inf')                          # one class never possible (no target holds it)
    logits[:, 4, 0] = float('-inf')                          # the blank impossible at one frame
    tg = torch.randint(1, 5, (3, 3), generator=g)
    return dict(lp=logits.log_softmax(-1), tg=tg, il=torch.tensor([12, 9, 12]), tl=torch.tensor([3, 2, 1]), w=torch.rand(3, generator=g) + 0.5)


# name -> (builder, (T, C, S), expected (forward path, backward path, state trips, class trips))
CTC = {
    # 63 states in one wave, every lane of the lattice live, labels distinct (every skip taken); il = T and tl = S
    'wave_full': (lambda: _ctc_inputs(32, 32, 31, [32, 31, 20], [31, 31, 10], 301, labels='distinct'), (32, 32, 31), ('wave', 'wave', 1, 1)),
    # T*C*4 == 60 KiB exactly: wave forward, general backward (its alpha comes from the other kernel); ~1600 nats
    'wave_lds_edge': (lambda: _ctc_inputs(480, 32, 31, [480, 401, 480], [31, 17, 30], 302), (480, 32, 31), ('wave', 'general', 1, 1)),
    # one frame and one label more: both general, 2S+1 = 65
    'general_just_over': (lambda: _ctc_inputs(481, 32, 32, [481, 377, 481], [32, 31, 9], 303), (481, 32, 32), ('general', 'general', 1, 1)),
    # 2S+3 = 1027 > 1024: the second trip of the state loops (3 states); tl = 512 reads out states 1023 / 1024, across the trip boundary
    'states_two_trips': (lambda: _ctc_inputs(540, 40, 512, [540, 530, 540], [512, 511, 300], 304, labels='no_adjacent_repeats'),
                         (540, 40, 512), ('general', 'general', 2, 1)),
    # T*C*4 > 60 KiB at 13 states: block 1024 from C, the class loop of the backward twice (76 classes in the second trip)
    'classes_two_trips': (lambda: _classes_two_trips(20, [20, 13, 20], [6, 4, 6], 305), (20, 1100, 6), ('general', 'general', 1, 2)),
    # the same C on the wave kernels
    'classes_wave': (lambda: _classes_two_trips(8, [8, 7, 8], [6, 3, 4], 306), (8, 1100, 6), ('wave', 'wave', 1, 1)),
    # logits x 3: ~7800 nats, occupancies by cancellation of large alpha + beta against nll
    'long_peaked': (lambda: _ctc_inputs(2000, 8, 30, [2000, 1337, 1], [30, 12, 1], 307, scale=3.0), (2000, 8, 30), ('general', 'general', 1, 1)),
    'repeats': (_repeats, (70, 6, 31), ('wave', 'wave', 1, 1)),
    'corners': (lambda: _corners(6), (12, 7, 6), ('wave', 'wave', 1, 1)),
    'corners_n1': (lambda: _corners(1), (12, 7, 6), ('wave', 'wave', 1, 1)),
    'masked': (_masked, (12, 6, 3), ('wave', 'wave', 1, 1)),
}


# ---------------------------------------------------------------------------------------------------------------------- head
SEED, STREAM, OFFSET = 0x1234ABCD5678, 2, 5        # the classifier's dropout stream (HALO_STREAM_CLASSIFIER) as tests/test_gpu_head.py draws it


def il_for(flen, r=0):
    """An input length whose feature length (ks 5, stride 4, pad 3: floor((il + 1) / 4) + 1) is ``flen``; r in 0..3 picks which."""
    return max(0, 4 * (flen - 1) - 1 + r)


def train_slices(B, H, cus=256):
    s = 1
    while s < 8 and (H // 32) % (2 * s) == 0 and B * 2 * s <= cus:
        s *= 2
    return s


def _head_inputs(B, T, H, V, S, p, flen, tl, seed, labels='random', wscale=1.0, fix=None):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, H, generator=g).relu()
    W = torch.randn(V, H, generator=g) / H ** 0.5 * wscale
    b = torch.randn(V, generator=g) * 0.1
    if labels == 'distinct':
        tg = torch.stack([torch.randperm(V - 1, generator=g)[:S] + 1 for _ in range(B)])
    else:
        tg = torch.randint(1, V, (B, S), generator=g)
    il = torch.tensor([il_for(f, i % 4) for i, f in enumerate(flen)], dtype=torch.int64)
    c = dict(feats=feats, W=W, b=b, tg=tg, il=il, tl=torch.tensor(tl, dtype=torch.int64), p=p, flen=list(flen))
    if fix:
        fix(c)
    return c


def head_mask(c):
    """The classifier dropout's multipliers from the oracle's Philox stream, [B,T,H] float32, or None without dropout."""
    from oracle import philox
    if c['p'] <= 0:
        return None
    return philox.dropout_mask(c['feats'].numel(), c['p'], SEED, STREAM, OFFSET).reshape(tuple(c['feats'].shape))


def _infeasible(c):
    c['tg'][1] = 1                                           # four equal labels need 7 frames; the row has 3
    c['il'][1] = 9


def _wide_flen():
    return [7 - (i % 3) for i in range(130)]


def _wide_tl():
    return [3 - (i % 4 == 3) for i in range(130)]


# name -> (builder, (B, T, H, V, S, p), slices per utterance on a 256-CU device)
HEAD = {
    # T = V = 32, 63 lattice states, the highest bit of the cmask words, labels distinct; flen 32 and 31 at tl = 31, one row tl = 10
    'tile_full': (lambda: _head_inputs(3, 32, 64, 32, 31, 0.0, [32, 31, 32], [31, 31, 10], 401, labels='distinct'), (3, 32, 64, 32, 31, 0.0), 2),
    'tile_full_drop': (lambda: _head_inputs(3, 32, 128, 32, 31, 0.5, [32, 31, 32], [31, 31, 10], 402, labels='distinct'), (3, 32, 128, 32, 31, 0.5), 4),
    # row 16 / class 16: the first of the train kernel's second pass over rows (tid >> 5) + 16 q
    'row16': (lambda: _head_inputs(2, 17, 64, 17, 8, 0.1, [17, 16], [8, 5], 403), (2, 17, 64, 17, 8, 0.1), 2),
    'smallest': (lambda: _head_inputs(2, 1, 64, 2, 1, 0.0, [1, 1], [1, 0], 404), (2, 1, 64, 2, 1, 0.0), 2),
    # 2 slices of 96 columns: 3 tiles, 6 k-steps for 8 waves
    'odd_tiles': (lambda: _head_inputs(2, 21, 192, 29, 10, 0.2, [21, 18], [10, 6], 405), (2, 21, 192, 29, 10, 0.2), 2),
    'odd_tiles_5': (lambda: _head_inputs(2, 21, 320, 32, 10, 0.0, [21, 19], [10, 7], 406), (2, 21, 320, 32, 10, 0.0), 2),
    'eight_slices': (lambda: _head_inputs(1, 21, 1024, 32, 10, 0.2, [21], [10], 407), (1, 21, 1024, 32, 10, 0.2), 8),
    # more utterances than half the CUs: one slice of 1536 columns (96 k-steps, 48 tiles: the job loop beyond two per wave)
    'one_slice_wide': (lambda: _head_inputs(130, 7, 1536, 32, 3, 0.1, _wide_flen(), _wide_tl(), 408), (130, 7, 1536, 32, 3, 0.1), 1),
    # W x 20: posteriors near 0 and 1, gradients by cancellation
    'peaked': (lambda: _head_inputs(3, 21, 256, 32, 10, 0.0, [21, 17, 21], [10, 10, 4], 409, wscale=20.0), (3, 21, 256, 32, 10, 0.0), 8),
    # row 1 infeasible, row 2 an empty target
    'with_infeasible': (lambda: _head_inputs(4, 21, 128, 9, 4, 0.0, [21, 3, 20, 19], [4, 4, 0, 2], 410, fix=_infeasible), (4, 21, 128, 9, 4, 0.0), 4),
}

GREEDY = ('tile_full', 'smallest', 'row16')
