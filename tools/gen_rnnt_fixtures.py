"""Write the two RNN-Transducer fixtures under tests/golden/ from a checkout of the reference (read at run time; nothing of it is kept):

  rnnt_config.json   the `model_config` mapping of examples/models/transducer/rnnt/small.yml.j2 rendered with
                     decoder_config.vocabsize = 1000 (settings only)
  rnnt_wiring.npz    the reference's OWN RnnTransducerEncoder, constructed and run over oracle/keras_shim.reference_runtime() at the tiny
                     size of tests/rnnt_cases.py: per setting ("ln": reductions [post, post, pre] by [3, 0, 2] with LayerNorm; "noln":
                     [pre, pre] by [2, 0] without) the weights under the reference's layer names ("<setting>|w|<path with | for />"), the
                     encoder output and its lengths; one ragged batch of log-mel features ("feats", "flen"); and for "ln" call_next over
                     the halves [0, 30) and [30, 80) of the batch with the carried states ("ln|next1", "ln|len1", "ln|states1", ... "2")

Usage: python tools/gen_rnnt_fixtures.py [--check]      (--check: the committed files equal a fresh run; writes nothing)
The reference tree is found where oracle/keras_shim.py looks for it.  The features carry the mask the model's FeatureExtraction layer
attaches (tests/rnnt_cases.py installs it on the input tensor): the encoder alone never builds one for a block without a `pre` reduction."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rnnt_cases as C  # noqa: E402
from oracle import keras_shim as KS  # noqa: E402
from render_deepspeech2_config import parse_block  # noqa: E402  (the indentation reader: needs neither jinja2 nor PyYAML)


def _quote_words(m):
    """[ post, post ] -> ["post", "post"]: the reader takes inline lists as JSON"""
    items = [v.strip() for v in m.group(1).split(",")]
    return "[" + ", ".join(v if re.fullmatch(r"-?[0-9.eE+-]+|True|False|true|false|null|\".*\"", v) else json.dumps(v) for v in items) + "]"


def render_config(vocabsize=1000):
    """the `model_config` block of small.yml.j2; its one template expression is the vocabulary size"""
    text = open(os.path.join(KS.REFERENCE_ROOT, "examples", "models", "transducer", "rnnt", "small.yml.j2")).read()
    text = re.sub(r"\{\{\s*decoder_config\.vocabsize\s*\}\}", str(int(vocabsize)), text)
    lines, take = [], False
    for ln in text.splitlines():
        if re.match(r"^\S", ln):
            take = ln.startswith("model_config:")
        if take:
            lines.append(re.sub(r"\[([^\[\]]*)\]", _quote_words, ln))
    return parse_block(lines)["model_config"]


def wiring():
    out = {}
    for setting in C.SETTINGS:
        cfg = C.tiny_config(setting)
        feats = C.features(C.audio(), cfg)
        run = C.reference_run(cfg, C.make_weights(cfg), feats, C.FLEN, split=C.SPLIT if setting == "ln" else None)
        assert run["lengths"].tolist() == C.ELEN[setting]
        if "feats" not in out:
            out["feats"], out["flen"] = feats, np.asarray(C.FLEN, np.int32)
        assert np.array_equal(out["feats"], feats)
        out.update({f"{setting}|w|" + k.replace("/", "|"): v for k, v in run["arrays"].items()})
        for k, v in run.items():
            if k != "arrays":
                out[f"{setting}|{k}"] = v
    return out


def main(check=False):
    conf, wire = render_config(), wiring()
    if check:
        with open(C.CONFIG_FIXTURE) as f:
            assert json.load(f) == conf, "rnnt_config.json differs from a fresh rendering"
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
