"""Drop-in for ha/recognizer.py: the CTC head (TemporalClassifier, recognizer.py:37-83) and the RNN transducer head (Transducer, :86-127)."""
import os

import torch
import torch.nn as nn

from . import _lib, functional as HF, ops
from .ctc import ctc_reduce_mean, ctc_viterbi
from .rnn import Decoder, DropoutStream
from .star import star_ctc_forward_score
from .transducer import BeamDecoder, GreedyDecoder, transducer_align, transducer_forward_score, transducer_loss


class TemporalClassifier(nn.Module):
    def __init__(self, feat_dim=1024, vocab_size=256):
        super().__init__()
        self.classifier = nn.Linear(feat_dim, vocab_size)
        self.dropout = nn.Dropout(0.2)
        self.dropout_stream = DropoutStream()

    def log_probs(self, features):
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.TemporalClassifier runs on the HIP device only')
        drop = self.dropout_stream.next(self.dropout.p, self.training)
        features = HF.dropout(features.float(), drop, _lib.HALO_STREAM_CLASSIFIER)
        logits = HF.linear(features, self.classifier.weight, self.classifier.bias)
        return HF.log_softmax(logits)

    def decode(self, features, input_lengths, target_lengths):
        # greedy, input_lengths ignored exactly like recognizer.py:48-59
        logits = self.log_probs(features)
        alignments, scores, hyp, hyp_len = ops.ctc_greedy(logits.detach().contiguous())
        lens = hyp_len.tolist()
        hypotheses = torch.nested.nested_tensor([hyp[i, :n] for i, n in enumerate(lens)])
        output_lengths = torch.tensor(lens)
        return hypotheses, output_lengths, alignments, scores, None

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
    hypothesis and keeps the whole n-best result of the last call as ``last_nbest``."""

    def __init__(self, feat_dim=1024, vocab_size=256):
        super().__init__()
        self.classifier = nn.Linear(feat_dim, vocab_size)
        self.lm = Decoder(vocab_size, emb_dim=512, hidden_dim=512, num_layers=2, dropout=0.2)
        self.dropout = nn.Dropout(0.2)
        self.dropout_stream = DropoutStream()
        self.fused_loss = os.environ.get('HALO_RNNT_LOSS_FUSED', '0') == '1'
        self.beam_size = int(os.environ.get('HALO_RNNT_BEAM', '0'))
        self.last_nbest = None

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

    def _decode_beam(self, features, input_lengths, N, capacity, width):
        """Beam search at ``width``: each row's best hypothesis in the five-value form (a merged hypothesis has no single alignment: the
        third value is [None] * N); ``last_nbest`` = (tokens [N, W, capacity], lengths [N, W], scores [N, W], counts [N])."""
        if width < 0:
            raise ValueError(f'Transducer.decode: beam_size {width} is negative')
        dec = getattr(self, '_beam_decoder', None)
        if dec is None or dec.max_batch < N or dec.capacity < capacity or dec.beam < width or dec._device != features.device:
            dec = BeamDecoder(self, max(N, dec.max_batch if dec else 0), max(capacity, dec.capacity if dec else 0),
                              max(width, dec.beam if dec else 0))
            self._beam_decoder = dec
        self.last_nbest = dec.decode(features, input_lengths, capacity, width)
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

    def forward(self, features, targets, input_lengths=None, target_lengths=None, star_penalty=None):   # star_penalty: ignored (:101)
        if not features.is_cuda:
            raise _lib.HaloError('haloop_amd.recognizer.Transducer runs on the HIP device only')
        dev = features.device
        N = features.shape[0]
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
