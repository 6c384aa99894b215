"""Test-infrastructure tooling: renders the reference's shipped model configs (examples/models/**/*.yml.j2, Jinja + YAML) and freezes
their `model_config` / `learning_config` mappings to tests/golden/reference_configs.json, so that the GPU box (which has no
/root/reference) can build models from the reference's own `class_name` + `config` (tests/test_dropin_api_gpu.py).

    python oracle/gen_config_fixture.py
    python oracle/gen_config_fixture.py --check     (the committed fixture is still the reference's rendering; writes nothing)
"""
import json
import os
import sys

import jinja2
import yaml

REF = "/root/reference/examples/models"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_configs.json")
FILES = {
    "transducer/conformer/small": "transducer/conformer/small.yml.j2",
    "transducer/conformer/small-streaming": "transducer/conformer/small-streaming.yml.j2",
    "ctc/conformer/small": "ctc/conformer/small.yml.j2",
    "transducer/contextnet/small": "transducer/contextnet/small.yml.j2",
}


def render(rel):
    txt = jinja2.Template(open(os.path.join(REF, rel)).read()).render(decoder_config={"vocabsize": 1000}, modeldir="/tmp/m",
                                                                      kaggle_model_handle="x", repodir=os.path.dirname(os.path.dirname(REF)),
                                                                      datadir="/tmp/d")
    return yaml.safe_load(txt)


def check():
    """model_config and learning_config.optimizer_config of every frozen entry equal a fresh rendering of its source."""
    frozen = json.load(open(OUT))
    assert sorted(frozen) == sorted(FILES), sorted(frozen)
    for key, v in frozen.items():
        doc = render(FILES[key])
        assert v["source"] == "examples/models/" + FILES[key], key
        assert doc["model_config"] == v["model_config"], key
        assert doc["learning_config"]["optimizer_config"] == v["learning_config"]["optimizer_config"], key
    print(OUT, "matches the reference's rendering:", sorted(frozen))


def main():
    out = {}
    for key, rel in FILES.items():
        doc = render(rel)
        lc = doc["learning_config"]
        out[key] = {"source": "examples/models/" + rel, "model_config": doc["model_config"],
                    "learning_config": {k: lc.get(k) for k in ("optimizer_config", "gwn_config", "gradn_config", "batch_size", "ga_steps")}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(OUT, {k: v["model_config"]["class_name"] for k, v in out.items()})


if __name__ == "__main__":
    check() if "--check" in sys.argv[1:] else main()
