"""What the encoders without a backward share (Jasper, DeepSpeech2, Transformer, RNN-T): the refusal of every training entry point, the
cache of constants derived from the weights, and the inference BatchNorm folded to an affine pair."""
import torch


class InferenceOnlyEncoder:
    """base of an encoder mixin that has no backward; goes in front of a head like every encoder (model.AsrModel's docstring)"""

    _BN_EPS = 1e-3  # keras.layers.BatchNormalization default
    _not_built = None  # the model's own sentence: which gradients do not exist

    def _init_encoder(self):
        super()._init_encoder()
        self._derived = {"epoch": -1}  # constants derived from the weights, per (name, type); shared with the f32 twin

    def _inference_only(self, *a, **k):
        raise NotImplementedError(f"{type(self).__name__} is inference only: {self._not_built} (weights arrive through load_weights)")

    train_step = loss_and_backward = compile = _inference_only

    def _encoder_length(self, t):
        return self.cfg.encoder_length(t)

    def frontend(self, signals, signals_length, training=False, masks=None):
        if training:
            self._inference_only()
        return self._features(signals, signals_length)

    def _features(self, signals, signals_length):
        """the feature map in inference mode: the base's front end unless the model has one of its own"""
        return super().frontend(signals, signals_length, False, None)

    # ------------------------------------------------------------------------------------------- constants derived from the weights
    def _cache(self):
        """the cache; dropped whenever the parameter store's weights change (load_weights, import_keras)"""
        d = self._derived
        if d["epoch"] != self.ps.epoch[0]:
            d.clear()
            d["epoch"] = self.ps.epoch[0]
        return d

    def _affine(self, bn):
        """inference BatchNorm `bn` (moving statistics) as (scale, shift), in f32; None -> (None, None)"""
        if bn is None:
            return None, None
        d, ps = self._cache(), self.ps
        aff = d.get((bn, "affine"))
        if aff is None:
            scale = (ps.p(bn + "/g") / torch.sqrt(ps.state[bn + "/mv"] + self._BN_EPS)).contiguous()
            shift = (ps.p(bn + "/b") - ps.state[bn + "/mm"] * scale).contiguous()
            aff = d[(bn, "affine")] = (scale, shift)
        return aff
