#!/usr/bin/env python3
"""Are the device kernels of two builds of libnefes_hip.so the same?  For a host-side refactor that must not move device code.
    python tools/kernels_identical.py [--allow-renames] <old.so> <new.so>
For every kernel of either library: its bytes in its code object's .text and its metadata note entry (vgpr / agpr / sgpr counts,
spill counts, private_segment_fixed_size, group_segment_fixed_size) must be equal, and so must the two sets of kernel names.
--allow-renames: a kernel only in the old library and one only in the new one with equal code bytes, size and notes are printed as
`renamed: old -> new` and are no difference (a refactor that renames kernels without touching them).
Prints every difference and the number of kernels compared; exit status 1 on any difference."""
import hashlib, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import BIN, code_objects

NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")


def kernels(lib):
    """{kernel name: (sha256 of its .text bytes, its note values)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            notes = subprocess.run([f"{BIN}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            meta = {}
            for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
                g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
                meta[g("name")] = tuple(g(k) for k in NOTE_KEYS)
            sec = subprocess.run([f"{BIN}/llvm-readelf", "-S", "-W", co], capture_output=True, text=True, check=True).stdout
            m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
            addr, off = int(m.group(1), 16), int(m.group(2), 16)
            data = open(co, "rb").read()
            syms = subprocess.run([f"{BIN}/llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
            here = {}                                   # (.dynsym and .symtab both list a kernel)
            for line in syms.splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC" and f[7] in meta:
                    a, size = int(f[1], 16), int(f[2])
                    here[f[7]] = (hashlib.sha256(data[off + a - addr: off + a - addr + size]).hexdigest(), size, meta[f[7]])
            missing = set(meta) - set(here)
            assert not set(here) & set(out), f"defined by two code objects of {lib}: {sorted(set(here) & set(out))[:3]}"
            out.update(here)
            assert not missing, f"kernels without a .text symbol: {sorted(missing)[:3]}"
    return out


def renames(old, new):
    """[(old name, new name)]: kernels that only one library has and whose code and notes are equal, paired in name order"""
    came = sorted(set(new) - set(old))
    pairs = []
    for o in sorted(set(old) - set(new)):
        same = [n for n in came if new[n] == old[o]]
        if same:
            pairs.append((o, same[0]))
            came.remove(same[0])
    return pairs


def main():
    args = [a for a in sys.argv[1:] if a != "--allow-renames"]
    old, new = kernels(args[0]), kernels(args[1])
    renamed = renames(old, new) if len(args) < len(sys.argv) - 1 else []
    for o, n in renamed:
        print(f"renamed: {o} -> {n}")
    bad = 0
    for name in sorted((set(old) | set(new)) - {x for pair in renamed for x in pair}):
        if name not in old or name not in new:
            print(f"only in {'new' if name in new else 'old'}: {name}")
            bad += 1
        elif old[name] != new[name]:
            what = "code" if old[name][:2] != new[name][:2] else "notes"
            print(f"{what} differ: {name}\n    old {old[name]}\n    new {new[name]}")
            bad += 1
    n = len(set(old) & set(new)) + len(renamed)
    print(f"{n} kernels compared ({sum(s for _, s, _ in new.values())} bytes of code in the new library): "
          + (f"{bad} DIFFERENCES" if bad else "code bytes and resource notes identical" + ("" if renamed else ", same set of names"))
          + (f", {len(renamed)} renamed" if renamed else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
