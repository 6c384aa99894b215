"""Data contract of the hot path — same NamedTuples (names, field order, meaning) as tensorflow_asr/schemas.py:20-62,
holding torch tensors instead of tf tensors."""
import math
import typing

import torch


class TrainInput(typing.NamedTuple):
    inputs: torch.Tensor  # [B, N] float32 PCM
    inputs_length: torch.Tensor  # [B] int32 samples
    predictions: torch.Tensor  # [B, U+1] int32, blank-prepended (tokenizers.py:165-167)
    predictions_length: torch.Tensor  # [B] int32


class TrainOutput(typing.NamedTuple):
    logits: torch.Tensor  # [B, T', U+1, V]
    logits_length: torch.Tensor  # [B] int32


class TrainLabel(typing.NamedTuple):
    labels: torch.Tensor  # [B, U] int32
    labels_length: torch.Tensor  # [B] int32


class TrainData(typing.NamedTuple):
    inputs: TrainInput
    labels: TrainLabel


class PredictInput(typing.NamedTuple):
    inputs: torch.Tensor
    inputs_length: torch.Tensor
    previous_tokens: typing.Optional[torch.Tensor] = None
    previous_encoder_states: typing.Optional[torch.Tensor] = None
    previous_decoder_states: typing.Optional[torch.Tensor] = None


class PredictOutput(typing.NamedTuple):
    tokens: torch.Tensor
    next_tokens: torch.Tensor
    next_encoder_states: typing.Optional[torch.Tensor] = None
    next_decoder_states: typing.Optional[torch.Tensor] = None


class AlignOutput(typing.NamedTuple):
    """Forced alignment of a batch (model.align): label u of utterance b is emitted at encoder frame frames[b, u]."""
    frames: torch.Tensor  # [B, U] int32: transducer = the frame that emits the label; CTC = the first frame in its state; -1 past the labels
    ends: typing.Optional[torch.Tensor]  # [B, U] int32, CTC only: one past the last frame in the label's state; None for the transducer
    label_log_probs: torch.Tensor  # [B, U] f32: log-probability the path gives the label (CTC: summed over its frames)
    scores: torch.Tensor  # [B] f32: log-probability of the best path (-inf: no path)
    seconds_per_frame: float  # time_reduction_factor * stride_ms / 1000


class RecognizeOutput(typing.NamedTuple):
    """Greedy recognition with token times and confidences (model.recognize_detailed).  frames / ends / log_probs / entropies are aligned
    column by column with predict.tokens: a transducer batch keeps recognize_batch's own layout (symbols from column 2), a single
    transducer utterance and CTC start at column 0; where no symbol sits, frames = ends = -1 and log_probs = entropies = 0."""
    predict: PredictOutput  # what recognize returns for the same input
    frames: torch.Tensor  # [B, W] int32: transducer = the encoder frame whose decision emitted the token; CTC = the first frame of its run
    ends: typing.Optional[torch.Tensor]  # [B, W] int32, CTC only: one past the last frame of the token's run; None for the transducer
    log_probs: torch.Tensor  # [B, W] f32: log-probability of the token (CTC: summed over the frames of its run)
    entropies: torch.Tensor  # [B, W] f32: entropy in nats of the distribution the token was chosen from (CTC: mean over its run)
    scores: torch.Tensor  # [B] f32: transducer = sum of the emitted tokens' log_probs; CTC = log-probability of the best path, blanks included
    seconds_per_frame: float  # time_reduction_factor * stride_ms / 1000
    vocab_size: int


class NBestOutput(typing.NamedTuple):
    """A beam search's n-best list with token times and confidences (model.recognize_nbest_detailed): every hypothesis aligned to the logits
    the search read.  frames / ends / log_probs / entropies are aligned column by column with tokens; where no token sits, frames = ends =
    -1 and log_probs = entropies = 0.  path(p) is hypothesis p as a RecognizeOutput."""
    search: tuple  # what recognize_nbest / recognize_nbest_lm return for the same input, untouched
    tokens: torch.Tensor  # [B, P, W] int32
    lengths: torch.Tensor  # [B, P] int32
    frames: torch.Tensor  # [B, P, W] int32: AlignOutput.frames of the hypothesis
    ends: typing.Optional[torch.Tensor]  # [B, P, W] int32, CTC only; None for a transducer
    log_probs: torch.Tensor  # [B, P, W] f32: AlignOutput.label_log_probs of the hypothesis
    entropies: torch.Tensor  # [B, P, W] f32: entropy in nats of the distribution the token was read from (CTC: mean over its frames)
    path_scores: torch.Tensor  # [B, P] f32: log-probability of the aligned path; -inf for a dead path, an over-long one, or one that does not fit
    seconds_per_frame: float
    vocab_size: int

    def path(self, p):
        """hypothesis p -> RecognizeOutput: token_times, token_confidences and word_details read it as they read a greedy result"""
        predict = PredictOutput(tokens=self.tokens[:, p], next_tokens=None, next_encoder_states=None, next_decoder_states=None)
        return RecognizeOutput(predict, self.frames[:, p], None if self.ends is None else self.ends[:, p], self.log_probs[:, p],
                               self.entropies[:, p], self.path_scores[:, p], self.seconds_per_frame, self.vocab_size)


def token_times(out):
    """Start time of every label in seconds, [B, U] f32 (-1 past the labels); AlignOutput or RecognizeOutput."""
    f = out.frames.to(torch.float32)
    return torch.where(out.frames >= 0, f * out.seconds_per_frame, torch.full_like(f, -1.0))


def token_confidences(out: RecognizeOutput, method="prob"):
    """Confidence in [0, 1] of every token, [B, W] f32, 0 where no token sits.  "prob": the token's probability, exp(log_prob / n_frames)
    with n_frames = ends - frames for CTC (the geometric mean over its run) and 1 for a transducer.  "entropy": 1 - H / ln(vocab_size)."""
    present = out.frames >= 0
    if method == "prob":
        n = (out.ends - out.frames).clamp(min=1).to(torch.float32) if out.ends is not None else torch.ones_like(out.log_probs)
        conf = torch.exp(out.log_probs / n)
    elif method == "entropy":
        conf = 1.0 - out.entropies / math.log(out.vocab_size)
    else:
        raise ValueError(f"token_confidences: method is 'prob' or 'entropy', not {method!r}")
    return torch.where(present, conf, torch.zeros_like(conf))


def word_details(out: RecognizeOutput, tokenizer, b):
    """Utterance b word by word: [(word, start_s, end_s, log_prob, confidence)] through tokenizer.word_spans.  end_s: the last token's `ends`
    (CTC) or its frame + 1 (transducer), in seconds; log_prob: summed over the word's tokens; confidence: its least sure token ("prob")."""
    tokens = out.predict.tokens[b].cpu()
    frames, lp = out.frames[b].cpu(), out.log_probs[b].cpu()
    ends = out.ends[b].cpu() if out.ends is not None else frames + 1
    conf = token_confidences(out, "prob")[b].cpu()
    words = []
    for word, first, last in tokenizer.word_spans(tokens.numpy()):
        cols = [k for k in range(first, last + 1) if int(frames[k]) >= 0]  # (a span may straddle columns that hold no token)
        if not cols:
            continue
        words.append((word, int(frames[cols[0]]) * out.seconds_per_frame, int(ends[cols[-1]]) * out.seconds_per_frame,
                      float(sum(float(lp[k]) for k in cols)), float(min(float(conf[k]) for k in cols))))
    return words
