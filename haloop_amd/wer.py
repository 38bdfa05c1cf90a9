"""Drop-in for ha/wer.py (`haw`: insertion / deletion / substitution counts and %WER) on the HIP edit-distance launch
(csrc/edit_distance.hip), where the reference aligns on the host through kaldialign and tabulates with pandas.

``edit_distance(hyp, hyp_lengths, ref, ref_lengths, group=1)`` is the device entry: batched Levenshtein distance with operation counts,
pair p scored against reference p // group -- ``group = W`` scores the [N, W, capacity] n-best lists ``transducer.BeamDecoder.decode``
returns against their rows' transcripts in one launch.  ``nbest_oracle`` picks each row's best hypothesis from those errors.

``clean_tokens`` / ``clean_and_join_tokens`` (ha/wer.py:10-15), ``word_errors`` (compute_wer_pointwise, :55-64, on lists of
``(key, text)`` in place of data frames) and ``format_wer`` (:67-73) are the text side.  The per-utterance ``tags`` string of `haw`
('.', 'X', '+', '-' per aligned position, :28-52) is not built: it needs the alignment itself, a backtrace, where the launch carries the
counts forward and keeps no back-pointers.  There is no command line and no pandas here.

The counts of a pair are those of one optimal alignment, chosen by the tie rule of include/halo.h (diagonal, then deletion, then
insertion); kaldialign breaks ties its own way, so ins / del / sub of a pair may be split differently where several alignments are
optimal -- their sum, the error count, is the same."""
import torch

from . import _lib, ops


def edit_distance(hyp, hyp_lengths, ref, ref_lengths, group=1):
    """hyp [P, Lh] tokens, hyp_lengths [P] (< 0: an absent hypothesis), ref [R, Lr], ref_lengths [R], P = R * group ->
    (errors [P] int32, counts [P, 3] int32 = (ins, del, sub)); an absent hypothesis gets errors -1 and counts 0.  Tokens at or past a
    length are never read (``-1`` padding is fine); ``hyp`` may be a strided view with unit stride along the tokens (a slice of a wider
    buffer, or [N, W, capacity], which is taken as N * W rows).  Up to ``ops.EDIT_DISTANCE_MAX_LEN`` tokens a side: wider tensors are
    refused by the library (``HaloError``), nothing is launched."""
    if not hyp.is_cuda or not ref.is_cuda:
        raise _lib.HaloError('haloop_amd.wer.edit_distance runs on the HIP device only (no CPU path)')
    dev = hyp.device
    if hyp.dim() == 3:
        hyp = hyp.reshape(-1, hyp.shape[2])
    if hyp.dim() != 2 or ref.dim() != 2:
        raise ValueError(f'edit_distance: hyp must be [P, Lh] (or [N, W, Lh]) and ref [R, Lr], got {tuple(hyp.shape)} and {tuple(ref.shape)}')
    hyp, ref = hyp.to(torch.int64), ref.to(device=dev, dtype=torch.int64)
    if hyp.shape[1] > 1 and hyp.stride(1) != 1 or hyp.shape[0] > 1 and hyp.stride(0) < hyp.shape[1]:
        hyp = hyp.contiguous()
    hl = hyp_lengths.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    rl = ref_lengths.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    return ops.edit_distance(hyp, hl, ref.contiguous(), rl, int(group))


def nbest_oracle(errors):
    """errors [N, W] (< 0: absent) -> (best_errors [N], best_index [N] int64): each row's fewest errors and the first hypothesis that
    has them; a row without a present hypothesis gets -1 and index 0."""
    big = torch.iinfo(errors.dtype).max
    keyed = torch.where(errors < 0, torch.full_like(errors, big), errors)
    best, index = keyed.min(dim=1)
    return torch.where(best == big, torch.full_like(best, -1), best), index


def clean_tokens(text):
    return ' '.join(token for token in text.split() if token != '␣')


def clean_and_join_tokens(text):
    return ''.join(token for token in text.split() if token != '␣').replace('▁', ' ')


def _word_ids(refs, hyps, join_bpe):
    """Host half of ``word_errors``: the pairs matched by key in the references' order (every hypothesis line of a key against every
    reference line of it, as the reference's merge does), their words as ids, padded with -1."""
    clean = clean_and_join_tokens if join_bpe else clean_tokens
    by_key = {}
    for key, text in hyps:
        by_key.setdefault(key, []).append(text)
    ids, keys, ref_rows, hyp_rows = {}, [], [], []
    for key, text in refs:
        for hyp_text in by_key.get(key, ()):
            keys.append(key)
            ref_rows.append([ids.setdefault(w, len(ids)) for w in clean(text).split()])
            hyp_rows.append([ids.setdefault(w, len(ids)) for w in clean(hyp_text).split()])

    def pad(rows):
        width = max([len(r) for r in rows] + [1])
        return [r + [-1] * (width - len(r)) for r in rows], [len(r) for r in rows]

    return keys, pad(ref_rows), pad(hyp_rows)


def word_errors(refs, hyps, join_bpe=False, device='cuda'):
    """refs, hyps: lists of ``(key, text)`` -- what `haw` reads from its two files, ``text`` a line's tokens -> one dict per matched pair,
    in the references' order: ``key``, ``ins``, ``del``, ``sub``, ``total``, ``ref_length``, ``hyp_length`` (compute_wer_pointwise's
    columns without ``tags``).  ``join_bpe``: `haw -w`, words from joined BPE pieces.  One ``edit_distance`` launch for all pairs."""
    keys, (ref_tok, ref_len), (hyp_tok, hyp_len) = _word_ids(refs, hyps, join_bpe)
    if not keys:
        return []
    errors, counts = edit_distance(torch.tensor(hyp_tok, device=device), torch.tensor(hyp_len, device=device),
                                   torch.tensor(ref_tok, device=device), torch.tensor(ref_len, device=device))
    errors, counts = errors.tolist(), counts.tolist()
    return [{'key': k, 'ins': c[0], 'del': c[1], 'sub': c[2], 'total': e, 'ref_length': rl, 'hyp_length': hl}
            for k, e, c, rl, hl in zip(keys, errors, counts, ref_len, hyp_len)]


def format_wer(rows, tag='WER'):
    """The summary tuple of ha/wer.py:67-73 over ``word_errors``'s rows."""
    total, ref_length = sum(r['total'] for r in rows), sum(r['ref_length'] for r in rows)
    ins, del_, sub = (sum(r[k] for r in rows) for k in ('ins', 'del', 'sub'))
    return f'%{tag}', round(100 * total / ref_length, 2), f'errors={total}/{ref_length}', f'ins={ins}', f'del={del_}', f'sub={sub}'
