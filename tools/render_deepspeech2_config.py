"""Render tests/golden/deepspeech2_config.json: the `model_config` mappings of the reference's examples/models/ctc/deepspeech2/base.yml.j2
and uni.yml.j2 with decoder_config.vocabsize = 1000 (settings only), as {"base": {...}, "uni": {...}}.
Usage: python tools/render_deepspeech2_config.py <directory holding base.yml.j2 and uni.yml.j2> [vocabsize]

Only the `model_config` block is read; its one template expression is the vocabulary size.  The mapping is parsed with a small
indentation reader (scalars, inline lists - nested ones included -, nested mappings, trailing comments) so the tool needs neither
jinja2 nor PyYAML."""
import json
import os
import re
import sys


def _scalar(v):
    v = re.sub(r"\s+#.*$", "", v).strip()
    if v.startswith("[") and v.endswith("]"):
        return json.loads(re.sub(r"\bTrue\b", "true", re.sub(r"\bFalse\b", "false", v)))
    if len(v) >= 2 and v[0] == v[-1] and v[0] in "\"'":
        return v[1:-1]
    if v in ("True", "true"):
        return True
    if v in ("False", "false"):
        return False
    if v in ("null", "~", ""):
        return None
    for cast in (int, float):
        try:
            return cast(v)
        except ValueError:
            pass
    return v


def parse_block(lines):
    root = {}
    stack = [(-1, root)]
    for ln in lines:
        if not ln.strip() or ln.lstrip().startswith("#"):
            continue
        ind = len(ln) - len(ln.lstrip())
        key, _, val = ln.strip().partition(":")
        while stack[-1][0] >= ind:
            stack.pop()
        if re.sub(r"#.*$", "", val).strip() == "":
            child = {}
            stack[-1][1][key] = child
            stack.append((ind, child))
        else:
            stack[-1][1][key] = _scalar(val)
    return root


def render(path, vocabsize=1000):
    text = open(path).read()
    text = re.sub(r"\{\{\s*decoder_config\.vocabsize\s*\}\}", str(int(vocabsize)), text)
    lines, take = [], False
    for ln in text.splitlines():
        if re.match(r"^\S", ln):
            take = ln.startswith("model_config:")
        if take:
            lines.append(ln)
    return parse_block(lines)["model_config"]


if __name__ == "__main__":
    vocab = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    out = {v: render(os.path.join(sys.argv[1], v + ".yml.j2"), vocab) for v in ("base", "uni")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "deepspeech2_config.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(dst)
