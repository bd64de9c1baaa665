#!/usr/bin/env python3
"""Records tests/golden/h3_instances.json: which instance of the fp16 two-part field kernels every entry point launches, or how it
refuses, over a grid of network descriptions -- taken from the dispatch code of the commit BEFORE the instance table
(csrc/field_h3_instances.h), so that tests/test_h3_instances.py holds the table's selectors to what the hand-written chains did.

    python tools/make_golden_h3_instances.py <recorder libnefes_hip.so> [out.json]

The recorder library is a scratch build of that earlier commit with ONE change, in csrc/field_fwd_h3.hip and csrc/field_bwd_h3.hip
each: the body of `launch_h3` / `launch_bwd_h3` (the one function template every dispatch path ends in) is replaced by

    snprintf(nefes_h3_recorded, sizeof nefes_h3_recorded, "%d|%s", <NEFES_TU_PART, or 0 where it is not defined>, __PRETTY_FUNCTION__);
    return 0;

with `__attribute__((weak)) char nefes_h3_recorded[512];` in front of the template (one buffer for all objects of the library).
No HIP call is left on any path, so this driver runs the real entry points -- their checks, nefes_blob_info, hg_geometry and the
`cls == 0 ? partA : partB` chains -- on the CPU with dummy non-null pointers, and reads which template instance in which object
they reached.  The patched sources are not kept; the golden is.

The grid (every cell is recorded, for every entry point): width x feat_dim x xyz_encoding x has_transient x fold_final x mode, with
one mode that is none of the three; entry points without a `mode` argument are recorded once per mode all the same."""
import ctypes as C
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AXES = {"width": [64, 128, 256, 512], "feat_dim": [0, 16, 29, 30, 128, 141, 142], "xyz_encoding": [0, 1], "has_transient": [0, 1],
        "fold_final": [0, 1], "mode": [0, 1, 2, 7]}
# request kind -> (backward, NEFES_H3_REQ_* flags of nefes_field_h3_instance)
REQUESTS = {"nefes_field_fwd_h3": (0, 0), "nefes_field_fwd_h3_zrow": (0, 16), "nefes_field_fwd_h3_hashgrid": (0, 4),
            "nefes_field_fwd_h3_fh": (0, 8), "nefes_field_fwd_train_h3": (0, 1), "nefes_field_fwd_train_h3_ext": (0, 3),
            "nefes_field_bwd_h3": (1, 0), "nefes_field_bwd_h3_hashgrid": (1, 4), "nefes_field_bwd_h3_fh": (1, 8),
            "nefes_field_bwd_static_h3": (1, 32), "nefes_field_bwd_train_h3": (1, 1), "nefes_field_bwd_train_h3_ext": (1, 3)}
MODE = {0: "SIGMA", 1: "STATIC", 2: "FULL", 3: "FULL_FOLD"}
ENC = {0: "FREQ10", 1: "EXTERNAL32", 2: "HASHGRID_FUSED"}
N, S = 3, 50


def instance_text(rec):
    """'5|int launch_h3(...) [MODE = 2, ENC = 0, W = 256, NTR = 5, TRAIN = false, FH = false]' -> 'fwd p5 <FULL,FREQ10,256,5,0,0>'"""
    part, pretty = rec.split("|", 1)
    v = {k: {"true": 1, "false": 0}.get(x, x) for k, x in re.findall(r"(\w+) = (\w+)", pretty[pretty.rindex("["):])}
    if "launch_bwd_h3" in pretty:
        kr = int(v["KR16"])
        kr = f"{kr & ~16} | NEFES_H3B_FOLD" if kr & 16 else str(kr)
        return f"bwd p{part} <{v['W']},{kr},{ENC[int(v['ENC'])]},{v['HAS_T']},{v['TRAIN']},{v['FH']}>"
    return f"fwd p{part} <{MODE[int(v['MODE'])]},{ENC[int(v['ENC'])]},{v['W']},{v['NTR']},{v['TRAIN']},{v['FH']}>"


def main():
    from nefes_amd import lib as L      # the argument lists only: the recorder library is bound here, not by lib.load()
    rec = C.CDLL(os.path.abspath(sys.argv[1]))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "h3_instances.json")
    recorded = (C.c_char * 512).in_dll(rec, "nefes_h3_recorded")
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)                         # every pointer argument: non-null, never dereferenced
    grid = L.NefesHashGridDesc(16, 2, 19, 16, 1.3819, 1.0)
    for name in REQUESTS:
        fn = getattr(rec, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]

    def call(name, d, mode):
        d = C.byref(d)
        g = C.byref(grid)
        return {
            "nefes_field_fwd_h3": lambda: rec.nefes_field_fwd_h3(d, p, mode, N, S, p, p, p, p, p, p, p, p, None),
            "nefes_field_fwd_h3_zrow": lambda: rec.nefes_field_fwd_h3_zrow(d, p, mode, N, S, p, p, p, p, p, p, None),
            "nefes_field_fwd_h3_hashgrid": lambda: rec.nefes_field_fwd_h3_hashgrid(d, p, g, p, mode, N, S, p, p, p, 0, p, p, p, None),
            "nefes_field_fwd_h3_fh": lambda: rec.nefes_field_fwd_h3_fh(d, p, mode, N, S, p, p, p, p, p, p, None),
            "nefes_field_fwd_train_h3": lambda: rec.nefes_field_fwd_train_h3(d, p, mode, N, S, p, p, p, p, p, p, p, p, None),
            "nefes_field_fwd_train_h3_ext": lambda: rec.nefes_field_fwd_train_h3_ext(d, p, mode, N, S, p, p, p, p, p, None),
            "nefes_field_bwd_h3": lambda: rec.nefes_field_bwd_h3(d, p, N, S, p, p, p, p, p, p, p, p, p, p, p, None),
            "nefes_field_bwd_h3_hashgrid": lambda: rec.nefes_field_bwd_h3_hashgrid(d, p, g, p, N, S, p, p, p, p, p, p, p, p, p, None),
            "nefes_field_bwd_h3_fh": lambda: rec.nefes_field_bwd_h3_fh(d, p, N, S, p, p, p, p, p, p, p, p, p, p, None),
            "nefes_field_bwd_static_h3": lambda: rec.nefes_field_bwd_static_h3(d, p, N, S, p, p, p, p, p, p, p, p, p, p, None),
            "nefes_field_bwd_train_h3": lambda: rec.nefes_field_bwd_train_h3(d, p, mode, N, S, p, p, p, p, p, p, p, p, p, p, None),
            "nefes_field_bwd_train_h3_ext": lambda: rec.nefes_field_bwd_train_h3_ext(d, p, mode, N, S, p, p, p, p, p, p, p, None),
        }[name]()

    outcomes, cells = [], {}
    for name in REQUESTS:
        cells[name] = []
        for w, c, enc, ht, fold, mode in itertools.product(*AXES.values()):
            recorded.value = b""
            rc = call(name, L.NefesNetDesc(w, c, ht, enc, fold), mode)
            text = recorded.value.decode()
            assert (rc == 0) == bool(text), (name, w, c, enc, ht, fold, mode, rc, text)
            o = f"{rc}|{instance_text(text) if text else ''}"
            if o not in outcomes:
                outcomes.append(o)
            cells[name].append(outcomes.index(o))
    doc = {"_": "python tools/make_golden_h3_instances.py: cells[request] = index into outcomes ('<return code>|<instance>') for "
                "itertools.product of the axes, in their order here",
           "axes": AXES, "requests": {k: list(v) for k, v in REQUESTS.items()}, "outcomes": outcomes, "cells": cells}
    with open(out, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('],"', '],\n"').replace('},"', '},\n"') + "\n")
    print(f"{out}: {sum(len(v) for v in cells.values())} cells, {len(outcomes)} outcomes")


if __name__ == "__main__":
    main()
