"""Data contract of the hot path — same NamedTuples (names, field order, meaning) as tensorflow_asr/schemas.py:20-62,
holding torch tensors instead of tf tensors."""
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


def token_times(out: AlignOutput):
    """Start time of every label in seconds, [B, U] f32 (-1 past the labels)."""
    f = out.frames.to(torch.float32)
    return torch.where(out.frames >= 0, f * out.seconds_per_frame, torch.full_like(f, -1.0))
