"""Writes tests/golden/curve_calls.json: what the twenty Encoder methods on a rate curve or a band curve hand to the C
library, return and refuse (tests/curve_calls.py says how it is taken; no GPU and no library needed).

It is a record of this project's own behaviour, written once from the tree BEFORE the twenty methods were folded onto
one implementation per operation, and not regenerated since: to check it, run this with --check on that parent commit.

Run from the repository root:  python tests/golden/make_curve_calls.py
                               python tests/golden/make_curve_calls.py --check   (compared with the committed file)
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, "curve_calls.json")

import audio_codec_amd as A        # noqa: E402
import curve_calls                 # noqa: E402

if __name__ == "__main__":
    doc = curve_calls.everything(A)                         # a line per case
    text = "{\n" + ",\n".join(
        f'"{kind}": {{\n' + ",\n".join(f"{json.dumps(label)}: {json.dumps(doc[kind][label], sort_keys=True)}"
                                       for label in sorted(doc[kind])) + "\n}" for kind in sorted(doc)) + "\n}\n"
    if "--check" in sys.argv[1:]:
        same = open(PATH).read() == text
        print("curve_calls.json:", "as committed" if same else "DIFFERS from what this tree does")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    print("wrote", PATH, len(text), "bytes")
