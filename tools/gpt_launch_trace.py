#!/usr/bin/env python3
"""Launch trace of the GPT block paths (haloop_amd/attention.py, lora.py, attention_audio.py): what a refactor of the Python above
libhalo must leave as it is.

For each case (the smallest shape that still takes the path, freshly seeded weights) every entry of ``_lib.SIGNATURES`` is wrapped on the
ctypes handle and each call becomes one line, in order: the entry's name and its arguments.  A pointer argument is written as the
index of its first appearance in the case (``p7``; NULL is ``0``; an array of pointers is the list of its elements' indices), so that a
launch that writes in place, or a backward launch that reads a tensor the forward kept, shows as such without comparing addresses.  While
a case runs, the result of every torch operator is kept alive (a TorchDispatchMode; the backward runs on the calling thread so that the
mode covers it): an address then names one tensor for the whole case and the indices do not depend on when Python drops a reference.
After the trace come the sha256 of every result tensor of the case (loss, per-token NLL, logits, every gradient).

    python tools/gpt_launch_trace.py --out DIR [--cases GLOB] [--tensors DIR2]     # DIR/<case>.trace, DIR/<case>.sha256
    python tools/gpt_launch_trace.py --compare DIR_A DIR_B [--tensors-a X --tensors-b Y]
    python tools/gpt_launch_trace.py --out DIR --no-gpu                            # the launch sequence alone, on a machine without a GPU

``--no-gpu``: every entry that launches returns success without launching (the host-side queries -- ``*_supported``, ``*_bytes``, the
math mode -- are the library's own) and tensors stay on the host, so the trace is the sequence the Python would issue and no hashes are
written.

``--tensors`` also saves the result tensors (torch.save, one file per case) so that ``--compare`` can give the max abs difference of a
tensor whose hashes differ (one that is summed with atomics is not bit-reproducible between two runs of the same code).
Run it on two checkouts on the same machine and compare: profiles/gpt_block_refactor_trace.md.
"""
import argparse
import contextlib
import ctypes
import fnmatch
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCHES = ('HALO_GPT_ROWS', 'HALO_GPT_ATTN_B16', 'HALO_GPT_DW_GROUP', 'HALO_GPT_GELU_EPILOGUE', 'HALO_GPT_DLN_B16', 'HALO_GPT_ROWMAJOR')


# ---- the trace ------------------------------------------------------------------------------------------------------------------------
class Trace:
    def __init__(self):
        self.lines, self.index, self.held = [], {}, []

    def pointer(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if v is None or v == 0:
            return '0'
        return 'p%d' % self.index.setdefault(int(v), len(self.index) + 1)

    def argument(self, v, ctype):
        if isinstance(v, ctypes.Array):
            if v._type_ is ctypes.c_void_p:
                return '[' + ' '.join(self.pointer(e) for e in v) + ']'
            return '[' + ' '.join(repr(e) for e in v) + ']'
        if ctype is ctypes.c_void_p:
            return self.pointer(v) if v is None or isinstance(v, (int, ctypes.c_void_p)) else '<ref>'
        if isinstance(v, (bytes, int, float)):
            return repr(v)
        return '<ref>'

    def call(self, name, args, argtypes):
        types = list(argtypes) + [None] * (len(args) - len(argtypes))
        self.lines.append(name + '(' + ', '.join(self.argument(a, t) for a, t in zip(args, types)) + ')')


@contextlib.contextmanager
def tracing(trace):
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from haloop_amd import _lib
    L = _lib.lib()
    orig = {n: getattr(L, n) for n in _lib.SIGNATURES}

    class KeepAll(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            trace.held.append(out)
            return out

    def wrap(n, fn):
        argtypes = _lib.SIGNATURES[n][1]

        def f(*a):
            trace.call(n, a, argtypes)
            return fn(*a)
        return f
    for n, fn in orig.items():
        setattr(L, n, wrap(n, fn))
    try:
        with torch.autograd.set_multithreading_enabled(False), KeepAll():
            yield trace
    finally:
        for n, fn in orig.items():
            setattr(L, n, fn)


def without_gpu():
    """Stubs for --no-gpu: launching entries of libhalo succeed without launching, ``.cuda()`` and device='cuda' stay on the host."""
    import torch
    from haloop_amd import _lib, ops
    torch.Tensor.cuda = torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.is_cuda = property(lambda self: True)
    torch.cuda.synchronize = torch.cuda.empty_cache = lambda *a, **k: None
    for name in ('empty', 'zeros', 'ones', 'full', 'randn', 'arange', 'tensor'):
        def on_host(*a, _f=getattr(torch, name), **k):
            if str(k.get('device', '')).startswith('cuda'):
                k['device'] = 'cpu'
            return _f(*a, **k)
        setattr(torch, name, on_host)
    L = _lib.lib()
    for n in _lib.SIGNATURES:
        if not n.endswith(('_supported', '_preferred', '_bytes', '_words')) and n not in ('halo_get_math_mode', 'halo_set_math_mode', 'halo_strerror'):
            setattr(L, n, lambda *a: 0)
    ops._stream = lambda: 0


def digest(t):
    import torch
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


# ---- models and batches -----------------------------------------------------------------------------------------------------------------
def make_gpt(C, H, L, V, T, bias=False, dropout=0.0, stable=False):
    import torch
    from haloop_amd import attention
    torch.manual_seed(0)
    cfg = attention.GPTConfig(block_size=T, vocab_size=V, n_layer=L, n_head=H, n_embd=C, bias=bias, dropout=dropout, stable_embedding=stable)
    model = attention.GPT(cfg)
    with torch.no_grad():                              # the reference's init zeroes wpe; give it content
        model.transformer.wpe.weight.normal_(0, 0.02)
    model.dropout_stream.seed = 0x5EED0D15EA5E
    return model.cuda()


def batch(B, T, V, keep=0.9):
    """ids, targets [B, T]: next-token targets, a fraction 1 - keep of them 0 (ignored)."""
    import torch
    g = torch.Generator().manual_seed(B * 1000003 + T * 101 + V)
    seq = torch.randint(1, V, (B, T + 1), generator=g)
    tg = seq[:, 1:].clone()
    tg[torch.rand(B, T, generator=g) >= keep] = 0
    return seq[:, :-1].contiguous().cuda(), tg.contiguous().cuda()


def train_step(model, ids, tg, out):
    model.train()
    for p in model.parameters():
        p.grad = None
    loss = model.forward_all(ids, tg)
    loss.backward()
    out['loss'] = loss
    for n, p in model.named_parameters():
        if p.grad is not None:
            out['grad.' + n] = p.grad


def score(model, ids, tg, out, train_mode=False):
    import torch
    model.train(train_mode)
    with torch.no_grad():
        out['nll'] = model.forward_all(ids, tg, reduction='none')


def add_lora(model, r, p):
    from haloop_amd import lora
    import torch
    torch.manual_seed(1)
    lora.attach_to_c_attn(model, r=r, lora_dropout=p)
    lora.mark_only_lora_as_trainable_(model)
    with torch.no_grad():                              # B starts at zero: give the adapter a term
        for blk in model.transformer.h:
            blk.attn.c_attn.lora_B.weight.normal_(0, 0.02)
    return model


# ---- the cases: name -> (math mode, switches, build() -> state, run(state, out)) ------------------------------------------------------
def cases():
    import torch
    from haloop_amd import generation
    table = {}

    def case(name, mode, build, run, env=None):
        table[name] = (mode, env or {}, build, run)

    # 128-tile forms: L = 2, C = 128, H = 4, V = 512, biases, dropout 0.1
    def small(stable, r=0, dropout=0.1):
        def build():
            m = make_gpt(128, 4, 2, 512, 64, bias=True, dropout=dropout, stable=stable)
            return add_lora(m, r, dropout) if r else m
        return build

    def infer(model, out, train_mode=False):
        """forward_all without and with ``past``, forward_context, forward with ``past``, Sampler.prefill and two general steps."""
        ids, tg = batch(2, 64, 512)
        model.train(train_mode)
        with torch.no_grad():
            out['nll'] = model.forward_all(ids, tg, reduction='none')
            out['context'], past = model.forward_context(ids[:, :40].contiguous())
            out['past'] = past
            out['nll_past'] = model.forward_all(ids[:, 40:].contiguous(), tg[:, 40:].contiguous(), past=past, reduction='none')
            out['logits_past'], out['present'] = model(ids[:, 40:41].contiguous(), past=past)
            sampler = generation.Sampler(model, 2, max_len=64)
            assert not sampler.fused
            out['prefill'] = sampler.prefill(ids[:, :16].contiguous()).clone()
            out['step1'] = sampler.step(ids[:, 16].contiguous()).clone()
            out['step2'] = sampler.step(ids[:, 17].contiguous()).clone()
            out['cache'] = sampler.cache

    for mode in ('f32', 'bf16x3'):
        for stable in (False, True):
            tag = f'tile-{mode}' + ('-stable' if stable else '')
            case(f'{tag}-train-2x64', mode, small(stable), lambda m, out: train_step(m, *batch(2, 64, 512), out))
            case(f'{tag}-train-1x32', mode, small(stable), lambda m, out: train_step(m, *batch(1, 32, 512), out))
            case(f'{tag}-infer', mode, small(stable), infer)

    # row forms: bf16, B = 8, T = 1024, L = 1, no bias
    def rows(H, V=2048, capacity=None, r=0, p=0.0):
        def build():
            m = make_gpt(512, H, 1, V, 1024)
            if r:
                add_lora(m, r, p)
            m.set_target_capacity(capacity)
            return m
        return build

    def row_pair(name, H=8, V=2048, capacity=None, env=None, keep=0.9):
        case(f'{name}-train', 'bf16', rows(H, V, capacity), lambda m, out: train_step(m, *batch(8, 1024, V, keep), out), env)
        case(f'{name}-score', 'bf16', rows(H, V, capacity), lambda m, out: score(m, *batch(8, 1024, V, keep), out), env)

    row_pair('rows-hd64', H=8)
    row_pair('rows-hd32', H=16)
    for sw, val in (('ROWS', '0'), ('ATTN_B16', '0'), ('DW_GROUP', '0'), ('GELU_EPILOGUE', '1'), ('DLN_B16', '1'), ('ROWMAJOR', '0')):
        row_pair(f'rows-hd64-{sw}={val}', env={'HALO_GPT_' + sw: val})
    row_pair('rows-hd64-V1000', V=1000)
    row_pair('rows-hd64-cap1536', capacity=1536, keep=0.15)       # about 1230 of 8192 rows carry a target

    # LoRA on c_attn, the base frozen
    for r in (4, 32):
        case(f'lora-r{r}-rows-train', 'bf16', rows(8, r=r, p=0.1), lambda m, out: train_step(m, *batch(8, 1024, 2048), out))
        # scoring with the adapter unmerged is train() mode, which takes no adapter dropout
        case(f'lora-r{r}-rows-score', 'bf16', rows(8, r=r, p=0.0), lambda m, out: score(m, *batch(8, 1024, 2048), out, train_mode=True))
    case('lora-r4-tile-bf16x3-train-2x64', 'bf16x3', small(False, r=4), lambda m, out: train_step(m, *batch(2, 64, 512), out))
    # (the adapter stays unmerged in train() mode, which scores only without dropout of either kind)
    case('lora-r4-tile-bf16x3-infer', 'bf16x3', small(False, r=4, dropout=0.0), lambda m, out: infer(m, out, train_mode=True))

    # AudioEncoder: the smallest configuration of tests/test_gpu_audio_encoder.py (g7_audio_encoder_tiny)
    def audio():
        import numpy as np
        from haloop_amd import attention, attention_audio
        g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'g7_audio_encoder_tiny.npz'))
        d_input, n_embd, n_head, n_layer, block, bias, vocab, B, T, S, seed = (int(v) for v in g['cfg'])
        torch.manual_seed(0)
        cfg = attention.GPTConfig(block_size=block, vocab_size=vocab, n_layer=n_layer, n_head=n_head, n_embd=n_embd, bias=bool(bias),
                                  causal=False, d_input=d_input, rotary_emb_dim=0, dropout=0.1)
        enc = attention_audio.AudioEncoder(cfg)
        enc.dropout_stream.seed = 0x5EED0D15EA5E
        x = torch.randn(B, T, d_input)
        il = torch.full((B,), T, dtype=torch.int64)
        return enc.cuda(), x.cuda(), il.cuda()

    def audio_infer(state, out):
        enc, x, il = state
        enc.eval()
        with torch.no_grad():
            out['feats'], out['lengths'], _ = enc(x, il)

    def audio_train(state, out):
        enc, x, il = state
        enc.train()
        feats, _, _ = enc(x, il)
        g = torch.Generator().manual_seed(5)
        feats.backward(torch.randn(feats.shape, generator=g).cuda())
        out['feats'] = feats
        for n, p in enc.named_parameters():
            if p.grad is not None:
                out['grad.' + n] = p.grad

    for mode in ('f32', 'bf16x3'):
        case(f'audio-{mode}-infer', mode, audio, audio_infer)
        case(f'audio-{mode}-train', mode, audio, audio_train)
    return table


def run_case(name, spec, out_dir, tensor_dir, hashes=True):
    import torch
    from haloop_amd import _lib
    mode, env, build, run = spec
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    _lib.set_math_mode(mode)
    _lib._scratch = None                               # every case lends the library its scratch anew: the trace of a case stands alone
    _lib.lend_scratch()
    state = build()
    torch.cuda.synchronize()
    out, trace = {}, Trace()
    with tracing(trace):
        run(state, out)
        torch.cuda.synchronize()
    tensors = {k: v.detach().cpu() for k, v in out.items()}
    with open(os.path.join(out_dir, name + '.trace'), 'w') as f:
        f.write('\n'.join(trace.lines) + '\n')
    if hashes:
        with open(os.path.join(out_dir, name + '.sha256'), 'w') as f:
            for k in sorted(tensors):
                f.write(f'{digest(tensors[k])}  {k}\n')
    if tensor_dir:
        torch.save(tensors, os.path.join(tensor_dir, name + '.pt'))
    for k in env:
        os.environ.pop(k, None)
    n = len(trace.lines)
    del trace, out, state
    torch.cuda.empty_cache()
    return n


def read_hashes(path):
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {line.split(None, 1)[1].strip(): line.split(None, 1)[0] for line in f if line.strip()}


def compare(dir_a, dir_b, tensors_a, tensors_b):
    """One line per case: launches, whether the traces are equal, the tensors whose hashes differ (with the max abs difference when both
    sides saved their tensors).  Exit status 1 when a trace differs."""
    names = sorted(n[:-6] for n in os.listdir(dir_a) if n.endswith('.trace'))
    bad = 0
    for name in names:
        a = open(os.path.join(dir_a, name + '.trace')).read().splitlines()
        pb = os.path.join(dir_b, name + '.trace')
        b = open(pb).read().splitlines() if os.path.exists(pb) else None
        same = a == b
        bad += not same
        line = f'{name}: {len(a)} calls, trace diff ' + ('empty' if same else 'NOT EMPTY')
        if not same and b is not None:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            line += f' (first at call {first}: {a[first] if first < len(a) else "-"} | {b[first] if first < len(b) else "-"})'
        ha = read_hashes(os.path.join(dir_a, name + '.sha256'))
        hb = read_hashes(os.path.join(dir_b, name + '.sha256')) if b is not None else {}
        differ = sorted(k for k in ha if hb.get(k) != ha[k])
        line += f'; {len(ha)} tensors, ' + ('no hashes' if not ha else 'all hashes equal' if not differ else f'{len(differ)} hashes differ')
        print(line)
        if differ and tensors_a and tensors_b:
            import torch
            ta, tb = torch.load(os.path.join(tensors_a, name + '.pt')), torch.load(os.path.join(tensors_b, name + '.pt'))
            for k in differ:
                d = (ta[k].double() - tb[k].double()).abs().max().item() if k in tb and ta[k].shape == tb[k].shape else float('nan')
                print(f'    {k}: max abs difference {d:.3e} (max abs value {ta[k].double().abs().max().item():.3e})')
        elif differ:
            print('    ' + ', '.join(differ))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--cases', default='*')
    ap.add_argument('--tensors')
    ap.add_argument('--no-gpu', action='store_true')
    ap.add_argument('--compare', nargs=2, metavar=('DIR_A', 'DIR_B'))
    ap.add_argument('--tensors-a')
    ap.add_argument('--tensors-b')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.tensors_a, args.tensors_b))
    if not args.out:
        ap.error('--out or --compare')
    os.makedirs(args.out, exist_ok=True)
    if args.tensors:
        os.makedirs(args.tensors, exist_ok=True)
    from haloop_amd import _lib
    _lib.lib()
    if args.no_gpu:
        without_gpu()
    for name, spec in cases().items():
        if fnmatch.fnmatch(name, args.cases):
            print(f'{name}: {run_case(name, spec, args.out, args.tensors, not args.no_gpu)} calls', flush=True)


if __name__ == '__main__':
    main()
