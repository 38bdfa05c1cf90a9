"""Drop-in for ha/ctc.py: the three CTC forward-score functions and ctc_reduce_mean, each a single
launch of the wave-per-utterance alpha kernel with the flags that reproduce that variant.

``ctc_viterbi`` is forced alignment, which the reference does not have: the best path of F.ctc_loss's lattice and its backtrace in one
launch (csrc/viterbi.hip).

``ctc_prefix_beam_search`` is CTC prefix beam search with exact merging, n-best lists from CTC emissions in the format of
``transducer.BeamDecoder.decode``: the whole batch in one launch (csrc/ctc_prefix_beam.hip).  ``PrefixBeamStream`` is
the same search over emissions that arrive in chunks, its beam carried in device memory between calls.
Both take a ``biasing.ContextGraph`` as ``context``: phrase boosts inside the same launch.
``haloop_amd.beam`` stays the reference's unmerged ha/beam.py."""
import torch

from . import _lib, ops

_SCORE3 = _lib.HALO_CTC_FULL_LATTICE | _lib.HALO_CTC_FINITE_MIN
_SCORE2 = _lib.HALO_CTC_FULL_LATTICE | _lib.HALO_CTC_NO_LEAD_BLANK_LOOP
_SCORE1 = _SCORE2 | _lib.HALO_CTC_WRAP_SKIP


def _single(emissions, targets, flags):
    T = emissions.shape[0]
    dev = emissions.device
    nll, _, _ = ops.ctc_fwd(emissions.float().contiguous()[:, None, :], True, targets[None].to(dev),
                            torch.tensor([T], device=dev), torch.tensor([targets.shape[0]], device=dev), flags)
    return nll[0]


def ctc_forward_score1(emissions, targets):
    """(T, C), (S,) -> scalar; ha/ctc.py:4-50 including its python-index wrap at s=1."""
    return _single(emissions, targets, _SCORE1)


def ctc_forward_score2(emissions, targets):
    """(T, C), (S,) -> scalar; ha/ctc.py:54-107."""
    return _single(emissions, targets, _SCORE2)


def ctc_forward_score3(emissions, targets, emission_lengths, target_lengths):
    """(T, N, C), (N, S), (N,), (N,) -> (N,); ha/ctc.py:110-174 (finfo.min as log zero)."""
    dev = emissions.device
    em = emissions.float()
    if em.stride(-1) != 1:
        em = em.contiguous()
    nll, _, _ = ops.ctc_fwd(em, True, targets.to(dev), emission_lengths.to(dev), target_lengths.to(dev), _SCORE3)
    return nll


def ctc_viterbi(emissions, targets, emission_lengths, target_lengths):
    """Forced alignment: emissions [T, N, C] log-probabilities (a strided view with a unit class stride is read in place, as
    ctc_forward_score3 reads it), targets [N, S], emission_lengths [N] (None: T), target_lengths [N] ->

        scores [N] float32       log-probability of the best alignment of the row's target, -inf when it has none
        alignments [N, T] int64  the label of every frame (0 = blank), -1 at frames past the row's length and in infeasible rows
        starts, ends [N, S] int32  first and last frame of every target token, -1 past the row's target length and in infeasible rows

    over the lattice of ``functional.ctc_loss``.  Among equally good paths the result is fixed by the tie rules of include/halo.h
    (stay, then s-1, then s-2; the final blank before the last label).  Not differentiable: the inputs are detached."""
    if not emissions.is_cuda:
        raise _lib.HaloError('haloop_amd.ctc.ctc_viterbi runs on the HIP device only (no CPU path)')
    dev = emissions.device
    em = emissions.detach().float()
    if em.dim() != 3:
        raise ValueError(f'ctc_viterbi: emissions must be [T, N, C], got {tuple(em.shape)}')
    if em.stride(-1) != 1:
        em = em.contiguous()
    targets = targets.detach().to(dev)
    S = targets.shape[1] if targets.dim() == 2 else -1
    if S == 0:                                            # no token anywhere: one padding column the kernel never reads
        targets = targets.new_zeros((targets.shape[0], 1))
    il = None if emission_lengths is None else emission_lengths.to(dev)
    scores, ali, starts, ends = ops.ctc_viterbi(em, True, targets, il, target_lengths.to(dev))
    return (scores, ali, starts[:, :0], ends[:, :0]) if S == 0 else (scores, ali, starts, ends)


def _check_context(context, V, name):
    """``context`` must be a ``biasing.ContextGraph`` over V classes."""
    from .biasing import ContextGraph
    if not isinstance(context, ContextGraph):
        raise ValueError(f'{name}: context must be a haloop_amd.biasing.ContextGraph')
    if context.vocab_size != V:
        raise ValueError(f'{name}: the context was compiled for {context.vocab_size} classes, the search has {V}')


def ctc_prefix_beam_search(emissions, emission_lengths=None, beam=4, capacity=None, context=None, return_parts=False):
    """CTC prefix beam search with exact merging ([Hannun14], Graves' prefix search; csrc/ctc_prefix_beam.hip), the whole
    batch in one launch: emissions [T, N, V] log-probabilities with class 0 the blank (a strided view with a unit class stride is read in
    place, so the head's ``log_probs.permute(1, 0, 2)`` costs no copy; they are not normalised here), emission_lengths [N] (None: T;
    clamped to [0, T]), ``beam`` = W from 1 to 16, ``capacity`` = the longest hypothesis, from 1 to T (None: T) ->

        tokens [N, W, capacity] int64   -1 past a hypothesis's length and in absent hypotheses
        lengths [N, W] int64            -1: an absent hypothesis
        scores [N, W] float32           log of the mass the search kept of the hypothesis, best first; -inf: absent
        counts [N] int64                hypotheses of the row

    the format of ``transducer.BeamDecoder.decode``, so ``wer.edit_distance(group=W)``, ``wer.nbest_oracle`` and
    ``transducer.nbest_risk`` take it as it is.  A member of the beam is a prefix with the masses of its alignments that end in blank and
    in its last label; per frame every member stays or is extended by every label, an extension that spells another member's prefix is
    merged into it, and the W best by (score descending, candidate position ascending) are kept: the definition and the tie rules are in
    include/halo.h.  The empty hypothesis is an ordinary member of the list; a row of no frames returns it alone, score 0.  Without
    pruning a score is ``-functional.ctc_loss(reduction='none')`` of its hypothesis, with pruning a lower bound.  Frames at or past a
    row's length are never read.  Not differentiable: the inputs are detached.

    ``context`` (a ``biasing.ContextGraph`` over V classes) biases the search towards its phrases inside the same one
    launch: a member also carries the state of the phrase automaton and the boost it holds, candidates rank by CTC mass + boost, and
    ``scores`` is that rank.  ``return_parts=True`` appends (boosts [N, W] float32, 0 where absent; states [N, W] int64, -1 where
    absent): ``scores - boosts`` is the CTC mass, ``scores - context.held.to(device)[states]`` settles the matches left open.  Without a
    context the parts are zeros and the root state."""
    if emissions.dim() != 3 or emissions.shape[0] < 1 or emissions.shape[1] < 1 or emissions.shape[2] < 2:
        raise ValueError(f'ctc_prefix_beam_search: emissions must be [T >= 1, N >= 1, V >= 2], got {tuple(emissions.shape)}')
    T, N, _ = emissions.shape
    W = int(beam)
    if W < 1 or W > ops.BEAM_MAX:
        raise ValueError(f'ctc_prefix_beam_search: beam {W} outside 1 .. {ops.BEAM_MAX}')
    cap = T if capacity is None else int(capacity)
    if cap < 1 or cap > T:
        raise ValueError(f'ctc_prefix_beam_search: capacity {cap} outside 1 .. T = {T}')
    if emission_lengths is not None and tuple(emission_lengths.shape) != (N,):
        raise ValueError(f'ctc_prefix_beam_search: emission_lengths must be [{N}]')
    if context is not None:
        _check_context(context, emissions.shape[2], 'ctc_prefix_beam_search')
    if not emissions.is_cuda:
        raise _lib.HaloError('haloop_amd.ctc.ctc_prefix_beam_search runs on the HIP device only (no CPU path)')
    em = emissions.detach().float()
    if em.stride(-1) != 1:
        em = em.contiguous()
    il = None if emission_lengths is None else emission_lengths.detach().to(em.device)
    if context is not None:
        out = ops.ctc_prefix_beam_biased(em, il, W, cap, context.to(em.device))
        return out if return_parts else out[:4]
    out = ops.ctc_prefix_beam(em, il, W, cap)
    if return_parts:
        present = out[1] >= 0
        return out + (torch.zeros_like(out[2]), present.to(torch.int64) - 1)
    return out


class PrefixBeamStream:
    """``ctc_prefix_beam_search`` over emissions that arrive in chunks (csrc/ctc_prefix_beam.hip): ``max_rows`` rows of
    a width-``beam`` search whose beam survives between calls, so after every call the n-best list of a row is what
    ``ctc_prefix_beam_search`` returns on the concatenation of the row's frames so far, bit for bit, at the cost of the new frames alone.
    ``capacity`` is the longest hypothesis of a stream (1 .. ``ops.PREFIX_BEAM_MAX_CAPACITY``), whatever the length of a chunk.  The state
    and the four outputs are allocated here, once.

    advance(emissions [T, N, V], n_frames=None, begin=None): row n takes its first clamp(n_frames[n], 0, T) frames (a device int32 /
        int64 tensor [N]; None: T) of the chunk, a strided view with a unit class stride read in place.  ``begin`` (a device bool / int32
        tensor [N]; None: no row) starts a row from the empty prefix, whatever it held, before its frames.  A row with no frames and no
        begin keeps its state and its n-best rows bit for bit.  Nothing is read from the device.  Returns (tokens [N, W, capacity],
        lengths [N, W], scores [N, W], counts [N]) in ``ctc_prefix_beam_search``'s format as views of this object's buffers: the next
        call overwrites them.  A row that never began holds no hypothesis (counts 0).
    nbest(): copies of the same four.
    ``context`` (a ``biasing.ContextGraph`` over ``vocab_size`` classes, kept by this object): the biased search of
        ``ctc_prefix_beam_search(context=...)``, still one launch per ``advance``; ``scores`` is then CTC mass + boost, and the buffers
        ``boosts`` [N, W] float32 and ``states`` [N, W] int64 are written with the other four.  parts(): copies of those two.
    Not differentiable: the inputs are detached."""

    def __init__(self, max_rows, vocab_size, beam=4, capacity=256, device='cuda', context=None):
        N, V, W, cap = int(max_rows), int(vocab_size), int(beam), int(capacity)
        if N < 1 or V < 2:
            raise ValueError(f'PrefixBeamStream: max_rows {N} and vocab_size {V} must be at least 1 and 2')
        if W < 1 or W > ops.BEAM_MAX:
            raise ValueError(f'PrefixBeamStream: beam {W} outside 1 .. {ops.BEAM_MAX}')
        if cap < 1 or cap > ops.PREFIX_BEAM_MAX_CAPACITY:
            raise ValueError(f'PrefixBeamStream: capacity {cap} outside 1 .. {ops.PREFIX_BEAM_MAX_CAPACITY}')
        if context is not None:
            _check_context(context, V, 'PrefixBeamStream')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _lib.HaloError('haloop_amd.ctc.PrefixBeamStream runs on the HIP device only (no CPU path)')
        nbytes = (ops.ctc_prefix_beam_state_bytes if context is None else ops.ctc_prefix_beam_biased_state_bytes)(V, W, cap)
        if nbytes == 0:
            raise ValueError(f'PrefixBeamStream: vocab_size {V} is more than the search takes')
        self.max_rows, self.vocab_size, self.beam, self.capacity = N, V, W, cap
        self.state = torch.zeros(N, nbytes, device=dev, dtype=torch.uint8)
        self.tokens = torch.full((N, W, cap), -1, device=dev, dtype=torch.int64)
        self.lengths = torch.full((N, W), -1, device=dev, dtype=torch.int64)
        self.scores = torch.full((N, W), float('-inf'), device=dev, dtype=torch.float32)
        self.counts = torch.zeros(N, device=dev, dtype=torch.int64)
        self.context = context
        if context is not None:
            self._tables = context.to(self.state.device)
            self.boosts = torch.zeros(N, W, device=dev, dtype=torch.float32)
            self.states = torch.full((N, W), -1, device=dev, dtype=torch.int64)

    def advance(self, emissions, n_frames=None, begin=None):
        N, V = self.max_rows, self.vocab_size
        if not torch.is_tensor(emissions) or emissions.dim() != 3 or emissions.shape[0] < 1 or tuple(emissions.shape[1:]) != (N, V):
            raise ValueError(f'PrefixBeamStream.advance: emissions must be [T >= 1, {N}, {V}]')
        for t, name, kinds in ((n_frames, 'n_frames', (torch.int32, torch.int64)), (begin, 'begin', (torch.bool, torch.int32))):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (N,) or t.dtype not in kinds):
                raise ValueError(f'PrefixBeamStream.advance: {name} must be a tensor [{N}] of ' + ' or '.join(str(k) for k in kinds))
        if not emissions.is_cuda or any(t is not None and not t.is_cuda for t in (n_frames, begin)):
            raise _lib.HaloError('haloop_amd.ctc.PrefixBeamStream runs on the HIP device only (no CPU path)')
        em = emissions.detach().float()
        if em.stride(-1) != 1:
            em = em.contiguous()
        nf = None if n_frames is None else n_frames.detach().clamp(0, em.shape[0]).to(torch.int32).contiguous()
        flags = None if begin is None else (begin.detach() != 0).to(torch.int32).mul_(ops.STREAM_BEGIN)
        self._launch(em, nf, flags)
        return self.tokens, self.lengths, self.scores, self.counts

    def _launch(self, em, nf, flags):
        """The one launch of a call: em [T, N, V] float32 with a unit class stride, nf and flags int32 [N] on the device or None."""
        if self.context is None:
            ops.ctc_prefix_beam_advance(em, nf, flags, self.beam, self.capacity, self.state, self.tokens, self.lengths, self.scores,
                                        self.counts)
        else:
            ops.ctc_prefix_beam_advance_biased(em, nf, flags, self.beam, self.capacity, self.state, self.tokens, self.lengths, self.scores,
                                               self.counts, self._tables, self.boosts, self.states)

    def nbest(self):
        return self.tokens.clone(), self.lengths.clone(), self.scores.clone(), self.counts.clone()

    def parts(self):
        if self.context is None:
            raise ValueError('PrefixBeamStream.parts: constructed without a context')
        return self.boosts.clone(), self.states.clone()


def ctc_reduce_mean(losses, target_lengths):
    return (losses / target_lengths).mean(-1)
