"""Write the two Transformer fixtures under tests/golden/ from a checkout of the reference (read at run time; nothing of it is kept):

  transformer_config.json   the `model_config` mappings of examples/models/ctc/transformer/base.yml.j2 and base-streaming.yml.j2 rendered
                            with decoder_config.vocabsize = 1000, as {"base": {...}, "base-streaming": {...}} (settings only)
  transformer_wiring.npz    the reference's OWN TransformerEncoder + TransformerDecoder, constructed and run over
                            oracle/keras_shim.reference_runtime() at the tiny size of tests/transformer_cases.py: the weights under the
                            reference's layer names ("w|<path with | for />"), one ragged batch of log-mel features ("feats", "flen"), and
                            per setting ("full" = every key, "chunked" = chunk 4 / history 8) the encoder output, its lengths and the logits

Usage: python tools/gen_transformer_fixtures.py [--check]      (--check: the committed files equal a fresh run; writes nothing)
The reference tree is found where oracle/keras_shim.py looks for it.  The shim has no dot-product attention core (only the relative
attention of the Conformer brought its own); tests/transformer_cases.py installs one on the runtime's keras.layers namespace."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import transformer_cases as C  # noqa: E402
from oracle import keras_shim as KS  # noqa: E402
from render_deepspeech2_config import render  # noqa: E402  (the indentation reader: needs neither jinja2 nor PyYAML)

YAMLS = ("base", "base-streaming")


def render_configs(vocabsize=1000):
    src = os.path.join(KS.REFERENCE_ROOT, "examples", "models", "ctc", "transformer")
    return {v: render(os.path.join(src, v + ".yml.j2"), vocabsize) for v in YAMLS}


def wiring():
    out = {}
    for setting in C.SETTINGS:
        ref = C.reference(setting)
        feats = ref["feats"].float().numpy()
        enc, elen, logits, arrays = C.reference_run(ref["cfg"], ref["W"], feats, ref["flen"])
        assert elen == C.ELEN
        if not out:
            out.update({"w|" + k.replace("/", "|"): v for k, v in arrays.items()})
            out["feats"], out["flen"] = feats, np.asarray(ref["flen"], np.int32)
        out[f"{setting}|encoder"], out[f"{setting}|lengths"], out[f"{setting}|logits"] = enc, np.asarray(elen, np.int32), logits
    return out


def main(check=False):
    conf, wire = render_configs(), wiring()
    if check:
        with open(C.CONFIG_FIXTURE) as f:
            assert json.load(f) == conf, "transformer_config.json differs from a fresh rendering"
        with np.load(C.WIRING) as z:
            assert sorted(z.files) == sorted(wire)
            for k in z.files:
                assert np.array_equal(z[k], wire[k]), k
        print("both fixtures equal a fresh run")
        return
    with open(C.CONFIG_FIXTURE, "w") as f:
        json.dump(conf, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(C.WIRING, "wb") as f:
        np.savez_compressed(f, **wire)
    print(C.CONFIG_FIXTURE, C.WIRING, os.path.getsize(C.WIRING), "bytes")


if __name__ == "__main__":
    main(check="--check" in sys.argv[1:])
