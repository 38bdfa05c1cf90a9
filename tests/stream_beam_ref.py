"""Float64 restatement, on the CPU in plain Python, of the carried CTC prefix beam search (haloop_amd.ctc.PrefixBeamStream,
halo_ctc_prefix_beam_advance), and the chunk schedules that tests/test_stream_beam_cpu.py and
tests/test_gpu_stream_beam.py share.  No tests in here.

The state of a row is its beam, a list of (tokens, pb, pnb) in beam order, None for a row that never began.  ``begin`` replaces it by the
empty prefix [((), 0, -inf)]; a frame is the frame of tests/ctc_prefix_beam_ref.py (stay candidates, extensions below the capacity, the
merge into stay candidates, the W best by (score descending, candidate position ascending)).  Nothing else is carried: the search of a
row's frames in any split into calls is the search of their concatenation.
"""
from ctc_prefix_beam_ref import NEG, lae


def frame(beam, et, capacity, W):
    """One frame: beam [(tokens, pb, pnb)] and the frame's V log-probabilities (a list of floats) -> the next beam."""
    total = [lae(pb, pnb) for _, pb, pnb in beam]
    cands = [[y, total[j] + et[0], pnb + et[y[-1]] if y else NEG] for j, (y, pb, pnb) in enumerate(beam)]
    stays = {c[0]: s for s, c in enumerate(cands)}
    for j, (y, pb, pnb) in enumerate(beam):
        if len(y) >= capacity:
            continue
        for k in range(1, len(et)):
            v = et[k] + (pb if y and k == y[-1] else total[j])
            s = stays.get(y + (k,))
            if s is None:
                cands.append([y + (k,), NEG, v])
            else:
                cands[s][2] = lae(cands[s][2], v)
    score = [lae(pb, pnb) for _, pb, pnb in cands]
    order = sorted((a for a in range(len(cands)) if score[a] > NEG), key=lambda a: (-score[a], a))
    return [tuple(cands[a]) for a in order[:W]]


class CarriedBeam:
    """N rows of the carried search at width W."""

    def __init__(self, N, W, capacity):
        self.N, self.W, self.capacity = N, W, capacity
        self.rows = [None] * N

    def begin(self, n):
        self.rows[n] = [((), 0.0, NEG)]

    def advance(self, e_chunk, n_frames=None, begin=None):
        """e_chunk [T, N, V] float64; n_frames: N ints or None (T), clamped to [0, T]; begin: N bools or None."""
        T = e_chunk.shape[0]
        for n in range(self.N):
            if begin is not None and begin[n]:
                self.begin(n)
            L = T if n_frames is None else max(0, min(int(n_frames[n]), T))
            for t in range(L):
                self.rows[n] = frame(self.rows[n], e_chunk[t, n].tolist(), self.capacity, self.W)

    def nbest(self, n):
        """[(tokens, score)] of row n, best first; [] for a row that never began."""
        return [(y, lae(pb, pnb)) for y, pb, pnb in (self.rows[n] or [])]


# ---- the chunk schedules: an int is a chunk length, a list the lengths of the calls in turn.  Each is the smallest that reaches what
#      its comment names. ----
SCHEDULES = {
    ('small', 4): (1, 2),             # the row of no frames, ragged rows (a row without frames in a later call), odd call lengths
    ('small', 1): (1, 2),
    ('rows17', 4): (5,),              # (the run that is compared with float64)
    ('rows17', 8): (5,),              # merges in the first frame after a boundary; more rows than any grouping
    ('rows17cap', 4): (4,),           # extensions refused at the capacity across boundaries
    ('long', 4): (7,),                # (the run that is compared with float64)
    ('long', 16): (7, [1, 64, 5]),    # both parities at a boundary, the frame loop past 64 inside one call
    ('wide', 3): (2,),                # V = 300
    ('stream', 3): (1,),              # emissions from L2
    ('deep', 16): (64,),              # token rows in the state, not in LDS; 7 calls
    ('huge', 2): (1,),                # 32-bit tokens
    ('tiny', 16): (1,),               # nothing pruned
}


def calls(T, spec):
    """-> [(offset, frames)] of the calls that cover T frames under ``spec``."""
    sizes = [spec] * ((T + spec - 1) // spec) if isinstance(spec, int) else list(spec)
    out, off = [], 0
    for s in sizes:
        out.append((off, min(s, T - off)))
        off += s
    assert off >= T and all(s > 0 for _, s in out)
    return out


def frames_of(lengths, off, size):
    """Row n's frames in the call at ``off``: clamp(L_n - off, 0, size)."""
    return [max(0, min(int(L) - off, size)) for L in lengths]
