"""The instance table of the fp16 two-part field kernels (nefes_amd/csrc/field_h3_instances.h) selects what the hand-written
dispatch chains before it selected (no GPU needed).

tests/golden/h3_instances.json was recorded from those chains (tools/make_golden_h3_instances.py: the entry points of the commit
before the table, run on the CPU with their launch template replaced by a recorder): for every entry point and every cell of a grid
of network descriptions, the instance launched -- the object part it is built in and its template arguments -- or the return code of
the refusal.  nefes_field_h3_instance answers the same question from the table's selectors; every cell must agree, NEFES_E_BADARG
and NEFES_E_UNSUPPORTED told apart, and a row moved to another part is a different answer."""
import ctypes as C
import itertools
import json
import os
import re

import pytest

from nefes_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the grid, restated (the golden must cover exactly this): 4 x 7 x 2 x 2 x 2 descriptions x 3 modes and one that is none of them
AXES = {"width": [64, 128, 256, 512], "feat_dim": [0, 16, 29, 30, 128, 141, 142],
        "xyz_encoding": [L.XYZ_FREQ10, L.XYZ_EXTERNAL32], "has_transient": [0, 1], "fold_final": [0, 1],
        "mode": [L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL, 7]}
T, X, H, F, Z, SB = L.H3_REQ_TRAIN, L.H3_REQ_EXT, L.H3_REQ_HASHGRID, L.H3_REQ_FH, L.H3_REQ_ZROW, L.H3_REQ_STATIC_BWD
# every fp16 entry point of include/nefes_hip.h: (backward, request flags)
REQUESTS = {"nefes_field_fwd_h3": (0, 0), "nefes_field_fwd_h3_zrow": (0, Z), "nefes_field_fwd_h3_hashgrid": (0, H),
            "nefes_field_fwd_h3_fh": (0, F), "nefes_field_fwd_train_h3": (0, T), "nefes_field_fwd_train_h3_ext": (0, T | X),
            "nefes_field_bwd_h3": (1, 0), "nefes_field_bwd_h3_hashgrid": (1, H), "nefes_field_bwd_h3_fh": (1, F),
            "nefes_field_bwd_static_h3": (1, SB), "nefes_field_bwd_train_h3": (1, T), "nefes_field_bwd_train_h3_ext": (1, T | X)}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "h3_instances.json")))


def table_rows():
    """The rows of both tables as nefes_field_h3_instance spells them, the NEFES_H3_HG_CLASS1 experiment rows left out."""
    src = open(os.path.join(ROOT, "nefes_amd", "csrc", "field_h3_instances.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"#ifdef NEFES_H3_HG_CLASS1.*?#else", "", src, flags=re.S)
    rows = []
    for d, macro in (("fwd", "NEFES_H3_FWD_INSTANCES"), ("bwd", "NEFES_H3_BWD_INSTANCES")):
        body = re.search(rf"#define {macro}\(X\)(.*?)\n\n", src, re.S).group(1)
        for args in re.findall(r"\bX\(([^()]*)\)", body):
            a = [x.strip() for x in args.split(",")]
            rows.append(f"{d} p{a[0]} <{','.join(a[1:])}>")
    return rows


def test_the_tables_are_the_listed_instances():
    rows = table_rows()
    fwd, bwd = [r for r in rows if r.startswith("fwd")], [r for r in rows if r.startswith("bwd")]
    assert len(fwd) == 30 and len(bwd) == 26 and len(set(rows)) == 56
    parts = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 15)
    count = lambda rs: [sum(r.split()[1] == f"p{p}" for r in rs) for p in parts]
    assert count(fwd) == [2, 5, 3, 4, 2, 2, 3, 2, 2, 1, 1, 1, 2]
    assert count(bwd) == [1, 3, 2, 4, 2, 2, 3, 2, 2, 1, 1, 1, 2]


def test_golden_covers_the_grid_and_every_row(golden):
    assert golden["axes"] == AXES
    assert {k: tuple(v) for k, v in golden["requests"].items()} == REQUESTS
    n_cells = len(list(itertools.product(*AXES.values())))
    assert n_cells == 896
    for name in REQUESTS:                                   # every grid cell has an entry
        assert len(golden["cells"][name]) == n_cells, name
        assert all(0 <= i < len(golden["outcomes"]) for i in golden["cells"][name])
    reached = {golden["outcomes"][i].split("|", 1)[1] for name in REQUESTS for i in golden["cells"][name]}
    assert reached - {""} == set(table_rows())              # every row is reached, and nothing outside the table is
    codes = {int(o.split("|")[0]) for o in golden["outcomes"]}
    assert codes == {0, -1, -2}                             # success, NEFES_E_BADARG, NEFES_E_UNSUPPORTED


def test_selection_replays_the_golden(golden):
    lib = L.load()
    name = C.create_string_buffer(96)
    wrong = []
    for req, (backward, flags) in REQUESTS.items():
        cells = golden["cells"][req]
        for i, (w, c, enc, ht, fold, mode) in enumerate(itertools.product(*AXES.values())):
            rc = lib.nefes_field_h3_instance(C.byref(L.NefesNetDesc(w, c, ht, enc, fold)), backward, mode, flags, name, len(name))
            got = f"{rc}|{name.value.decode()}"
            if got != golden["outcomes"][cells[i]]:
                wrong.append((req, dict(width=w, feat_dim=c, xyz_encoding=enc, has_transient=ht, fold_final=fold, mode=mode),
                              got, golden["outcomes"][cells[i]]))
    assert not wrong, f"{len(wrong)} of {len(REQUESTS) * 896} cells differ (request, cell, got, golden): {wrong[:5]}"


def test_flags_that_name_no_entry_point():
    lib = L.load()
    name = C.create_string_buffer(96)
    d = L.NefesNetDesc(256, 16, 1, L.XYZ_FREQ10, 0)
    for backward, flags in ((0, SB), (1, Z), (0, X), (0, H | F), (0, T | Z), (1, T | SB), (0, 64)):
        assert lib.nefes_field_h3_instance(C.byref(d), backward, L.FIELD_FULL, flags, name, len(name)) == -1, (backward, flags)
        assert name.value == b""
    assert lib.nefes_field_h3_instance(None, 0, L.FIELD_FULL, 0, name, len(name)) == -1
    assert lib.nefes_field_h3_instance(C.byref(d), 0, L.FIELD_FULL, 0, None, 0) == -1
