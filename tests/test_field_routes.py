"""Which kernel serves which field pass (ops.field_route and the launchers, Functions and predicates built on it), on the CPU:
tools/make_golden_field_routes.py replays every case of its grid -- pack kind x shape x encoding x transient x stale fp16 streams x
fold, NEFES_SPLIT x NEFES_X6, mode x direction x input kind, a small sample count and one at the 32-bit bound, plus the predicates
of ops.py / train.py / field.py -- and each outcome (entry points and timer keys in launch order, or the exception's class) must
equal the one recorded in tests/golden/field_routes.json, case by case."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_field_routes as G      # noqa: E402


def test_field_routes_match_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "field_routes.json")) as f:
        rec = json.load(f)
    wrong, ids = [], []
    with G.patched():
        for k, (cid, thunk) in enumerate(G.cases()):
            ids.append(cid)
            got = thunk()
            want = rec["outcomes"][rec["cases"][k]] if k < rec["n"] else "<no such case in the fixture>"
            if got != want:
                wrong.append(f"{cid}\n    recorded: {want}\n    now:      {got}")
    assert len(ids) == rec["n"] == len(rec["cases"])
    assert hashlib.sha256("\n".join(ids).encode()).hexdigest() == rec["ids_sha256"], "the case list differs from the recorded one"
    assert not wrong, f"{len(wrong)} of {len(ids)} routes changed:\n" + "\n".join(wrong[:40])


def test_patches_are_undone():
    from nefes_amd import lib as L
    from nefes_amd import ops
    before = (L.load, ops._chk, ops._stream, ops._timed, ops.SPLIT, ops.USE_X6)
    with G.patched():
        G.set_switches({"SPLIT": "f32", "USE_X6": False})
    assert (L.load, ops._chk, ops._stream, ops._timed, ops.SPLIT, ops.USE_X6) == before
