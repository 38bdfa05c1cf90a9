"""Drop-in for ha/recognizer.py: the CTC head (TemporalClassifier, recognizer.py:37-83) and the RNN transducer head (Transducer, :86-127)."""
import os

import torch
import torch.nn as nn

from . import _lib, functional as HF, ops, wer
from .ctc import _check_context, ctc_prefix_beam_search, ctc_reduce_mean, ctc_viterbi
from .fusion import CTCFusionDecoder, TransducerFusionDecoder
from .rnn import Decoder, DropoutStream
from .star import star_ctc_forward_score
from .transducer import BeamDecoder, GreedyDecoder, nbest_risk, transducer_align, transducer_forward_score, transducer_loss


class TemporalClassifier(nn.Module):
    """The CTC head (ha/recognizer.py:37-83).

    ``beam_size`` (HALO_CTC_BEAM when the head is built; a caller may set the attribute or pass ``decode(..., beam_size=W)``): 0, the
    default, decodes greedily as the reference does; W >= 1 runs ``ctc.ctc_prefix_beam_search`` at that width, returns
    each row's best hypothesis and keeps the whole n-best result of the last call as ``last_nbest``.

    ``mwer_beam`` (HALO_CTC_MWER when the head is built; a caller may set the attribute): 0, the default, leaves ``forward`` as it is;
    W >= 1 makes ``forward`` of a head in training mode return ``mwer_forward(..., beam_size=W)``, minimum-word-error-rate fine-tuning
    on the n-best lists of the prefix search.

    ``set_lm(lm, lm_weight, insertion_bonus)`` fuses an ``rnn.Decoder`` language model into the search of ``decode`` at a width
    W >= 1 (``fusion.CTCFusionDecoder``); ``set_lm(None)`` takes it out again.  The LM is no submodule of the head:
    ``state_dict()``, ``parameters()``, ``to()`` and ``train()`` do not see it.

    ``set_context(graph)`` biases the search of ``decode`` at a width W >= 1 towards the phrases of a ``biasing.ContextGraph`` inside its
    one launch; ``set_context(None)`` takes it out again.  Like the LM it is no submodule."""

    def __init__(self, feat_dim=1024, vocab_size=256):
        super().__init__()
        self.classifier = nn.Linear(feat_dim, vocab_size)
        self.dropout = nn.Dropout(0.2)
        self.dropout_stream = DropoutStream()
        self.beam_size = int(os.environ.get('HALO_CTC_BEAM', '0'))
        self.mwer_beam = int(os.environ.get('HALO_CTC_MWER', '0'))
        self.last_nbest = None
        self.last_parts = None
        self._fusion = None    # None, or a dict (not a module: the LM stays out of this head's parameters and state_dict)
        self._context = None   # None, or a biasing.ContextGraph

    def set_lm(self, lm, lm_weight=0.5, insertion_bonus=0.0):
        """Fuse ``lm`` (an ``rnn.Decoder`` over this head's classes, in eval mode, on the device; the caller moves it) into
        ``decode(beam_size=W >= 1)``: candidates rank by their CTC mass + lm_weight * log P_LM + insertion_bonus * length, ``last_nbest``
        holds the fused lists and ``last_parts`` their (ctc_scores, lm_scores).  ``set_lm(None)`` restores the unfused search.  Greedy
        decoding and ``mwer_forward`` do not use the LM."""
        if lm is None:
            self._fusion, self.last_parts = None, None
            return
        V = self.classifier.out_features
        if getattr(lm, 'num_classes', None) != V:
            raise ValueError(f'TemporalClassifier.set_lm: the LM has {getattr(lm, "num_classes", None)} classes, the head {V}')
        CTCFusionDecoder(lm, 1, 1, 1, lm_weight, insertion_bonus)      # the argument checks, now and not at the first decode
        self._fusion = {'lm': lm, 'lm_weight': float(lm_weight), 'insertion_bonus': float(insertion_bonus), 'decoder': None}

    def set_context(self, graph):
        """Bias ``decode(beam_size=W >= 1)`` towards the phrases of ``graph`` (a ``biasing.ContextGraph`` over this head's classes):
        candidates rank by their CTC mass + the boost of the phrase they are spelling, ``last_nbest`` holds the biased lists and
        ``last_parts`` their (ctc_scores, boosts).  ``set_context(None)`` restores the unbiased search.  Greedy decoding, ``mwer_forward``
        and ``align`` do not use the context.  A head with both an LM and a context refuses ``decode(beam_size >= 1)``: biasing inside
        the fused search is not built."""
        if graph is None:
            self._context, self.last_parts = None, None
            return
        _check_context(graph, self.classifier.out_features, 'TemporalClassifier.set_context')
        self._context = graph

    def log_probs(self, features):
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.TemporalClassifier runs on the HIP device only')
        drop = self.dropout_stream.next(self.dropout.p, self.training)
        features = HF.dropout(features.float(), drop, _lib.HALO_STREAM_CLASSIFIER)
        logits = HF.linear(features, self.classifier.weight, self.classifier.bias)
        return HF.log_softmax(logits)

    def decode(self, features, input_lengths, target_lengths, beam_size=None):
        width = self.beam_size if beam_size is None else int(beam_size)
        if width:
            return self._decode_beam(features, input_lengths, width)
        # greedy, input_lengths ignored exactly like recognizer.py:48-59
        logits = self.log_probs(features)
        alignments, scores, hyp, hyp_len = ops.ctc_greedy(logits.detach().contiguous())
        lens = hyp_len.tolist()
        hypotheses = torch.nested.nested_tensor([hyp[i, :n] for i, n in enumerate(lens)])
        output_lengths = torch.tensor(lens)
        return hypotheses, output_lengths, alignments, scores, None

    def _decode_beam(self, features, input_lengths, width):
        """Prefix beam search at ``width`` on this head's ``log_probs``, honouring ``input_lengths`` (None: T), with room for T symbols:
        each row's best hypothesis in the five-value form ``Transducer._decode_beam`` returns (a merged hypothesis has no single
        alignment: the third value is [None] * N); ``last_nbest`` = (tokens [N, W, T], lengths [N, W], scores [N, W], counts [N])."""
        if width < 0:
            raise ValueError(f'TemporalClassifier.decode: beam_size {width} is negative')
        if self.training:
            raise NotImplementedError('TemporalClassifier.decode(beam_size >= 1) is an inference path: put the head in eval mode')
        N = features.shape[0]
        fusion, context = getattr(self, '_fusion', None), getattr(self, '_context', None)
        if fusion is not None and context is not None:
            raise NotImplementedError('TemporalClassifier.decode: contextual biasing inside the LM-fused search (fusion.CTCFusionDecoder) '
                                      'is not built: take out the LM (set_lm(None)) or the context (set_context(None))')
        with torch.no_grad():
            logits = self.log_probs(features)
            if context is not None:
                *nbest, boosts, _ = ctc_prefix_beam_search(logits.permute(1, 0, 2), input_lengths, width, context=context, return_parts=True)
                self.last_nbest = tuple(nbest)
                self.last_parts = (torch.where(nbest[1] >= 0, nbest[2] - boosts, nbest[2]), boosts)     # (-inf stays -inf where absent)
            elif fusion is None:
                self.last_nbest = ctc_prefix_beam_search(logits.permute(1, 0, 2), input_lengths, width)
            else:
                if width > ops.BEAM_MAX:
                    raise ValueError(f'TemporalClassifier.decode: beam_size {width} outside 1 .. {ops.BEAM_MAX}')
                T, dec = logits.shape[1], fusion['decoder']
                if dec is None or dec.max_batch < N or dec.capacity < T or dec.beam < width \
                        or dec._device != fusion['lm'].embedding.weight.device:       # an LM moved since needs new buffers
                    dec = CTCFusionDecoder(fusion['lm'], max(N, dec.max_batch if dec else 0), max(T, dec.capacity if dec else 0),
                                           max(width, dec.beam if dec else 0))
                    fusion['decoder'] = dec
                self.last_nbest = dec.decode(logits.permute(1, 0, 2), input_lengths, T, width, fusion['lm_weight'], fusion['insertion_bonus'])
                self.last_parts = dec.last_parts
        tokens, lengths, scores, _ = self.last_nbest
        lens = lengths[:, 0].tolist()                           # every row returns at least one hypothesis
        hypotheses = torch.nested.nested_tensor([tokens[i, 0, :max(n, 0)] for i, n in enumerate(lens)])
        return hypotheses, torch.tensor(lens), [None] * N, scores[:, 0].clone(), None

    def _search_nbest(self, features, input_lengths, capacity, width):
        """The search of ``mwer_forward``: under ``no_grad``, on the head in eval mode (no dropout, and nothing drawn from the dropout
        stream); every module's mode is put back, also when the search raises."""
        modes = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            with torch.no_grad():
                return ctc_prefix_beam_search(self.log_probs(features).permute(1, 0, 2), input_lengths, width, capacity)
        finally:
            for m, mode in modes:
                m.training = mode

    def mwer_forward(self, features, targets, input_lengths, target_lengths, beam_size=4, mle_weight=0.01):
        """Minimum-word-error-rate training on n-best lists, the CTC twin of ``Transducer.mwer_forward`` ([Prabhavalkar18]; DESIGN.md
        3.3o, 3.3p) -> (loss, info):

            the W = beam_size best hypotheses of every row by ``ctc.ctc_prefix_beam_search`` (no gradient, the head in eval mode for the
                search, the features undropped, room for min(T, target_lengths.max() + 1) symbols);
            their error counts against ``targets`` by ``wer.edit_distance``;
            their losses -log P(hypothesis | x) by ``functional.ctc_loss(reduction='none')`` on N * W rows: the hypotheses (padding and
                absent hypotheses as token 0, absent ones with length 0) against W views of the row's log-probabilities, which
                ``forward``'s dropout stream, classifier and log-softmax produce;
            loss = mean_n ``transducer.nbest_risk``(losses, errors)[n] (+ mle_weight x the CTC loss of ``forward`` on the same
                log-probabilities, unless mle_weight is 0).

        ``info``: ``nbest`` (the search's tuple), ``errors`` [N, W] int32, ``risk`` [N] and ``nbest_losses`` [N, W], detached.  The empty
        hypothesis is an ordinary member of a CTC n-best list (length 0, present).  The N * W views of the log-probabilities are
        materialised once (W x their size; the lattice kernels take no group argument); their gradient is summed over W by the view's
        backward, not by an index-add.  Every launch on the path is deterministic."""
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.TemporalClassifier runs on the HIP device only')
        dev = features.device
        N, T, W = features.shape[0], features.shape[1], int(beam_size)
        targets, il, tl = targets.to(dev), input_lengths.to(dev), target_lengths.to(dev)
        nbest = self._search_nbest(features, il, min(T, int(tl.max()) + 1), W)
        tokens, lengths = nbest[0], nbest[1]                                             # [N, W, cap] (-1 padded), [N, W] (-1: absent)
        errors, _ = wer.edit_distance(tokens, lengths, targets, tl, group=W)
        errors = errors.view(N, W)

        logits = self.log_probs(features)                                                # (N, T, C)
        V = logits.shape[2]
        hyps = tokens.clamp(min=0).view(N * W, -1)
        rows = logits[:, None].expand(N, W, T, V).reshape(N * W, T, V)
        losses = HF.ctc_loss(rows.permute(1, 0, 2), hyps, il[:, None].expand(N, W).reshape(-1), lengths.clamp(min=0).view(-1),
                             reduction='none').view(N, W)
        risk = nbest_risk(losses, errors)
        loss = risk.mean()
        if mle_weight != 0:
            loss = loss + mle_weight * HF.ctc_loss(logits.permute(1, 0, 2), targets, il, tl)
        return loss, {'nbest': nbest, 'errors': errors, 'risk': risk.detach(), 'nbest_losses': losses.detach()}

    def align(self, features, targets, input_lengths=None, target_lengths=None):
        """Forced alignment of ``targets`` [N, S] to the frames of ``features`` [N, T, feat_dim] (lengths default to T and S as in
        ``forward``): ``ctc.ctc_viterbi`` on this head's ``log_probs`` -> (scores [N], alignments [N, T], starts [N, S], ends [N, S]).
        An inference path (eval mode only: alignment under dropout is not built); the reference has no aligner."""
        if self.training:
            raise NotImplementedError('TemporalClassifier.align is an inference path: put the head in eval mode')
        N = features.shape[0]
        if target_lengths is None:
            target_lengths = torch.full((N,), targets.shape[1], dtype=torch.long)
        with torch.no_grad():
            logits = self.log_probs(features)
            return ctc_viterbi(logits.permute(1, 0, 2), targets, input_lengths, target_lengths)

    def forward(self, features, targets, input_lengths=None, target_lengths=None, star_penalty=None,
                measure_entropy=False):
        if input_lengths is None:
            input_lengths = torch.full((features.shape[0],), features.shape[1], dtype=torch.long)
        if target_lengths is None:
            target_lengths = torch.full((features.shape[0],), len(targets), dtype=torch.long)
        if self.mwer_beam > 0 and self.training and star_penalty is None:
            return self.mwer_forward(features, targets, input_lengths, target_lengths, beam_size=self.mwer_beam)
        logits = self.log_probs(features)
        if star_penalty is not None:
            # recognizer.py:74-82: the star-CTC branch reads self.star_penalty, which the reference's constructor never sets (so it raises
            # AttributeError unless the caller has assigned the attribute); same here, through the same attribute access
            dev = logits.device
            losses = star_ctc_forward_score(logits.permute(1, 0, 2), targets.to(dev), input_lengths.to(dev), target_lengths.to(dev),
                                            star_penalty=self.star_penalty)
            return ctc_reduce_mean(losses, target_lengths.to(dev)), {}
        logits1 = logits.permute(1, 0, 2)                     # T, N, C (a view; the kernel takes strides)
        dev = logits.device
        loss = HF.ctc_loss(logits1, targets.to(dev), input_lengths.to(dev), target_lengths.to(dev))
        return loss, {}


class Transducer(nn.Module):
    """RNN transducer head of the `rnn-transducer` arch (ha/recognizer.py:86-127, ha/init.py:180-185): an LSTM prediction network over
    the zero-prefixed targets, a linear transcription head on the (dropped-out) encoder features, the additive joint, and the
    transducer loss.  The reference's live branch calls torchaudio's ``rnnt_loss(joint, ..., blank=0, reduction='mean',
    fused_log_softmax=True)`` (:121-126); torchaudio is not part of this build, and the loss here is the same quantity through the
    reference's own lattice: mean over the batch of ``transducer_forward_score(joint.log_softmax(-1), ...)`` -- the equality the
    reference's tests assert (ha/transducer.py:210-231, 234-268) -- on the HIP lattice kernels, differentiable end to end.

    ``fused_loss`` (HALO_RNNT_LOSS_FUSED=1 when the head is built; a caller may set the attribute): the same losses from
    ``transducer.transducer_loss`` on the two factors of the joint, which builds no [N, T, U+1, V] tensor.  Off by
    default.

    ``beam_size`` (HALO_RNNT_BEAM when the head is built; a caller may set the attribute or pass ``decode(..., beam_size=W)``): 0, the
    default, decodes greedily; W >= 1 runs ``transducer.BeamDecoder`` at that width, returns each row's best
    hypothesis and keeps the whole n-best result of the last call as ``last_nbest``.

    ``mwer_beam`` (HALO_RNNT_MWER when the head is built; a caller may set the attribute): 0, the default, leaves ``forward`` as it is;
    W >= 1 makes ``forward`` of a head in training mode return ``mwer_forward(..., beam_size=W)``, minimum-word-error-rate fine-tuning
    on the n-best lists of the beam search.

    ``set_fusion_lm(lm, lm_weight, insertion_bonus)`` fuses an ``rnn.Decoder`` language model into the search of ``decode`` at a width
    W >= 1 (``fusion.TransducerFusionDecoder``); ``set_fusion_lm(None)`` takes it out again.  (``self.lm`` is the
    prediction network, hence the name.)  The fusion LM is no submodule of the head: ``state_dict()``, ``parameters()``, ``to()`` and
    ``train()`` do not see it."""

    def __init__(self, feat_dim=1024, vocab_size=256):
        super().__init__()
        self.classifier = nn.Linear(feat_dim, vocab_size)
        self.lm = Decoder(vocab_size, emb_dim=512, hidden_dim=512, num_layers=2, dropout=0.2)
        self.dropout = nn.Dropout(0.2)
        self.dropout_stream = DropoutStream()
        self.fused_loss = os.environ.get('HALO_RNNT_LOSS_FUSED', '0') == '1'
        self.beam_size = int(os.environ.get('HALO_RNNT_BEAM', '0'))
        self.mwer_beam = int(os.environ.get('HALO_RNNT_MWER', '0'))
        self.last_nbest = None
        self.last_parts = None
        self._fusion = None    # None, or a dict (not a module: the fusion LM stays out of this head's parameters and state_dict)

    def set_fusion_lm(self, lm, lm_weight=0.5, insertion_bonus=0.0):
        """Fuse ``lm`` (an ``rnn.Decoder`` over this head's classes, in eval mode, on the device; the caller moves it) into
        ``decode(beam_size=W >= 1)``: candidates rank by their transducer mass + lm_weight * log P_LM + insertion_bonus * length,
        ``last_nbest`` holds the fused lists and ``last_parts`` their (rnnt_scores, lm_scores).  ``set_fusion_lm(None)`` restores the
        unfused search.  Greedy decoding, ``mwer_forward`` and ``align`` do not use the LM."""
        if lm is None:
            self._fusion, self.last_parts = None, None
            return
        TransducerFusionDecoder(self, lm, 1, 1, 1, lm_weight, insertion_bonus)      # the argument checks, now and not at the first decode
        self._fusion = {'lm': lm, 'lm_weight': float(lm_weight), 'insertion_bonus': float(insertion_bonus), 'decoder': None}

    def decode(self, features, input_lengths, condtarget_lengths=None, prompt=None, beam_size=None):
        """The ``Decodable`` call (ha/recognizer.py:12-34, as ha/loop.py:295-303 makes it): greedy transducer search with room for
        ``condtarget_lengths.max() + 1`` symbols per row (the length guide ha/transformer.py:128 takes) ->
        (hypotheses nested_tensor, output_lengths, frames [N, capacity] (-1 past a row's length), scores, None), in the form
        TemporalClassifier.decode returns its five values.  The search itself is ``transducer.GreedyDecoder``, kept on the module."""
        if condtarget_lengths is None:
            # the reference's own two-argument signature, which raises there too (recognizer.py:92-93): no length guide
            raise NotImplementedError('Transducer.decode needs condtarget_lengths (capacity = condtarget_lengths.max() + 1); '
                                      'for a capacity of your own use haloop_amd.transducer.GreedyDecoder')
        if prompt is not None:
            raise NotImplementedError('Transducer.decode: prompts are not built')
        if self.training:
            raise NotImplementedError('Transducer.decode is an inference path: put the head in eval mode')
        N, capacity = features.shape[0], int(condtarget_lengths.max()) + 1
        width = self.beam_size if beam_size is None else int(beam_size)
        if width:
            return self._decode_beam(features, input_lengths, N, capacity, width)
        dec = getattr(self, '_greedy_decoder', None)
        if dec is None or dec.max_batch < N or dec.capacity < capacity or dec._state.device != features.device:
            dec = GreedyDecoder(self, max(N, dec.max_batch if dec else 0), max(capacity, dec.capacity if dec else 0))
            self._greedy_decoder = dec
        tokens, lengths, frames, scores, _ = dec.decode(features, input_lengths, capacity)
        lens = lengths.tolist()
        hypotheses = torch.nested.nested_tensor([tokens[i, :n] for i, n in enumerate(lens)])
        return hypotheses, torch.tensor(lens), frames, scores, None

    def _beam_decoder_for(self, features, N, capacity, width):
        """The head's ``BeamDecoder``, rebuilt when a call needs more room than it has (or another device)."""
        dec = getattr(self, '_beam_decoder', None)
        if dec is None or dec.max_batch < N or dec.capacity < capacity or dec.beam < width or dec._device != features.device:
            dec = BeamDecoder(self, max(N, dec.max_batch if dec else 0), max(capacity, dec.capacity if dec else 0),
                              max(width, dec.beam if dec else 0))
            self._beam_decoder = dec
        return dec

    def _decode_beam(self, features, input_lengths, N, capacity, width):
        """Beam search at ``width``: each row's best hypothesis in the five-value form (a merged hypothesis has no single alignment: the
        third value is [None] * N); ``last_nbest`` = (tokens [N, W, capacity], lengths [N, W], scores [N, W], counts [N])."""
        if width < 0:
            raise ValueError(f'Transducer.decode: beam_size {width} is negative')
        fusion = getattr(self, '_fusion', None)
        if fusion is None:
            self.last_nbest = self._beam_decoder_for(features, N, capacity, width).decode(features, input_lengths, capacity, width)
        else:
            if width > ops.BEAM_MAX:
                raise ValueError(f'Transducer.decode: beam_size {width} outside 1 .. {ops.BEAM_MAX}')
            dec = fusion['decoder']
            if dec is None or dec.max_batch < N or dec.capacity < capacity or dec.beam < width or dec._device != features.device:
                dec = TransducerFusionDecoder(self, fusion['lm'], max(N, dec.max_batch if dec else 0),
                                              max(capacity, dec.capacity if dec else 0), max(width, dec.beam if dec else 0))
                fusion['decoder'] = dec
            self.last_nbest = dec.decode(features, input_lengths, capacity, width, fusion['lm_weight'], fusion['insertion_bonus'])
            self.last_parts = dec.last_parts
        tokens, lengths, scores, _ = self.last_nbest
        lens = lengths[:, 0].tolist()                           # every row returns at least one hypothesis
        hypotheses = torch.nested.nested_tensor([tokens[i, 0, :n] for i, n in enumerate(lens)])
        return hypotheses, torch.tensor(lens), [None] * N, scores[:, 0].clone(), None

    def align(self, features, targets, input_lengths, target_lengths, prompt=None):
        """Forced alignment of ``targets`` [N, U]: the prediction network over the zero-prefixed targets and the classifier exactly as
        ``forward`` runs them, then ``transducer.transducer_align`` on the two factors of the joint -> (scores [N], frames [N, U]: the
        frame at which every target token is emitted, -1 past a row's target length).  An inference path (eval mode only)."""
        if prompt is not None:
            raise NotImplementedError('Transducer.align: prompts are not built')
        if self.training:
            raise NotImplementedError('Transducer.align is an inference path: put the head in eval mode')
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.Transducer runs on the HIP device only')
        dev = features.device
        N = features.shape[0]
        with torch.no_grad():
            targets = targets.to(dev)
            lm_targets = torch.cat([targets.new_zeros((N, 1)), targets], dim=1)
            lm_outputs, _ = self.lm.forward_batch_first(lm_targets, self.lm.init_hidden(N))
            feats = HF.linear(features.float(), self.classifier.weight, self.classifier.bias)
            return transducer_align(feats, lm_outputs, targets, input_lengths.to(dev), target_lengths.to(dev))

    def _search_nbest(self, features, input_lengths, capacity, width):
        """The beam search of ``mwer_forward``: under ``no_grad``, on the head in eval mode (the decoders refuse a training head); every
        module's mode is put back, also when the search raises."""
        modes = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            with torch.no_grad():
                return self._beam_decoder_for(features, features.shape[0], capacity, width).decode(features, input_lengths, capacity, width)
        finally:
            for m, mode in modes:
                m.training = mode

    def mwer_forward(self, features, targets, input_lengths, target_lengths, beam_size=4, mle_weight=0.01):
        """Minimum-word-error-rate training on n-best lists ([Prabhavalkar18], [Guo20]) -> (loss, info):

            the W = beam_size best hypotheses of every row by ``transducer.BeamDecoder`` (no gradient, the head in eval mode for the search,
                the features undropped, room for target_lengths.max() + 1 symbols as in ``decode``);
            their error counts against ``targets`` by ``wer.edit_distance``;
            their losses -log P(hypothesis | x) by ``transducer.transducer_loss`` on N * W rows: the prediction network over the
                zero-prefixed hypotheses (padding and absent hypotheses as token 0, absent ones with length 0) against W views of the
                row's ``feats``, which ``forward``'s dropout stream and classifier produce;
            loss = mean_n ``transducer.nbest_risk``(losses, errors)[n] (+ mle_weight x the fused transducer loss of the reference, from
                the same ``feats``, unless mle_weight is 0).

        ``info``: ``nbest`` (the search's tuple: tokens [N, W, capacity], lengths [N, W], scores [N, W], counts [N]), ``errors`` [N, W]
        int32, ``risk`` [N] and ``nbest_losses`` [N, W], detached.  The N * W views of ``feats`` are materialised once (W x the size of
        ``feats``; the joint kernels take no group argument); their gradient is summed over W by the view's backward, not by an
        index-add.  The prediction network takes its embedding gradient in token order (``ordered_grad``), not by the float atomics of the
        ordinary lookup, so the whole step is bit-reproducible.  Rows with an input length of 0 are refused as in ``transducer_loss``."""
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.Transducer runs on the HIP device only')
        dev = features.device
        N, W = features.shape[0], int(beam_size)
        targets, il, tl = targets.to(dev), input_lengths.to(dev), target_lengths.to(dev)
        nbest = self._search_nbest(features, il, int(tl.max()) + 1, W)
        tokens, lengths = nbest[0], nbest[1]                                             # [N, W, cap] (-1 padded), [N, W] (-1: absent)
        errors, _ = wer.edit_distance(tokens, lengths, targets, tl, group=W)
        errors = errors.view(N, W)

        drop = self.dropout_stream.next(self.dropout.p, self.training)
        feats = HF.dropout(features.float(), drop, _lib.HALO_STREAM_CLASSIFIER)
        feats = HF.linear(feats, self.classifier.weight, self.classifier.bias)          # (N, T, C)
        T, V = feats.shape[1], feats.shape[2]
        hyps = tokens.clamp(min=0).view(N * W, -1)
        lm_hyps = torch.cat([hyps.new_zeros((N * W, 1)), hyps], dim=1)
        lm_outputs, _ = self.lm.forward_batch_first(lm_hyps, self.lm.init_hidden(N * W), ordered_grad=True)
        rows = feats[:, None].expand(N, W, T, V).reshape(N * W, T, V)
        losses = transducer_loss(rows, lm_outputs, hyps, il[:, None].expand(N, W).reshape(-1), lengths.clamp(min=0).view(-1)).view(N, W)
        risk = nbest_risk(losses, errors)
        loss = risk.mean()
        if mle_weight != 0:
            lm_targets = torch.cat([targets.new_zeros((N, 1)), targets], dim=1)
            ref_outputs, _ = self.lm.forward_batch_first(lm_targets, self.lm.init_hidden(N), ordered_grad=True)
            loss = loss + mle_weight * transducer_loss(feats, ref_outputs, targets, il, tl).mean()
        return loss, {'nbest': nbest, 'errors': errors, 'risk': risk.detach(), 'nbest_losses': losses.detach()}

    def forward(self, features, targets, input_lengths=None, target_lengths=None, star_penalty=None):   # star_penalty: ignored (:101)
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.Transducer runs on the HIP device only')
        dev = features.device
        N = features.shape[0]
        if self.mwer_beam > 0 and self.training:
            return self.mwer_forward(features, targets, input_lengths, target_lengths, beam_size=self.mwer_beam)
        targets = targets.to(dev)
        hidden = self.lm.init_hidden(N)
        lm_targets = torch.cat([targets.new_zeros((N, 1)), targets], dim=1)              # input needs to start with 0 (:107)
        lm_outputs, _ = self.lm.forward_batch_first(lm_targets, hidden)                 # (N, U1, C)
        drop = self.dropout_stream.next(self.dropout.p, self.training)
        feats = HF.dropout(features.float(), drop, _lib.HALO_STREAM_CLASSIFIER)
        feats = HF.linear(feats, self.classifier.weight, self.classifier.bias)          # (N, T, C)
        if self.fused_loss:
            return transducer_loss(feats, lm_outputs, targets, input_lengths.to(dev), target_lengths.to(dev)).mean(), {}
        joint = feats[:, :, None, :] + lm_outputs[:, None, :, :]                        # (N, T, U1, C): a broadcast add (glue)
        losses = transducer_forward_score(HF.log_softmax(joint), targets, input_lengths.to(dev), target_lengths.to(dev))
        return losses.mean(), {}
