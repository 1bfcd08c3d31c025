#!/usr/bin/env python3
"""Do two builds ship the same device code?  For every gfx9xx code object inside two libraries (or object files) this compares,
per function symbol, the bytes in .text (by symbol address and size) and, per kernel, its entry in the AMDGPU metadata note
(register counts, LDS and scratch bytes, spill counts, arguments).  Whole code objects never compare equal -- each carries a
per-compilation id symbol -- so the comparison is by symbol.  No GPU, no ROCm tools.
    python tools/code_object_diff.py OLD NEW        OLD, NEW: libl3d_hip.so or a translation unit's .o
prints the counts and three lists (differing, only in OLD, only in NEW); exit status 1 if any of the three is non-empty.
--allow-removed REGEX: symbols only in OLD that match it are listed and do not fail (a change that drops instantiations)."""
import argparse
import re
import struct
import sys

import msgpack

try:
    from tools.kernel_meta import _code_objects, _notes
except ImportError:                                  # run as a script from tools/
    from kernel_meta import _code_objects, _notes


def _functions(elf):
    """{symbol: bytes} of every function symbol that lies in .text"""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    names = [elf[stroff + s[0]:elf.index(b"\0", stroff + s[0])].decode() for s in secs]
    text = names.index(".text")
    taddr, toff, tsize = secs[text][3:6]
    out = {}
    for s in secs:
        if s[1] != 2:                                # SHT_SYMTAB
            continue
        symstr = secs[s[6]][4]                       # sh_link: its string table
        for p in range(s[4], s[4] + s[5], 24):
            name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, p)
            if info & 15 != 2 or shndx != text:      # STT_FUNC
                continue
            assert taddr <= value and value + size <= taddr + tsize, "symbol outside .text"
            sym = elf[symstr + name:elf.index(b"\0", symstr + name)].decode()
            out[sym] = elf[toff + value - taddr:toff + value - taddr + size]
    return out


def device_code(path):
    """{symbol: [(text bytes, kernel metadata or None), ...]}: a list, since two translation units may hold a symbol of one name"""
    out = {}
    for _triple, elf in _code_objects(open(path, "rb").read()):
        meta = {}
        for name, ntype, desc in _notes(elf):
            if name == "AMDGPU" and ntype == 32:
                for k in msgpack.unpackb(desc, raw=False, strict_map_key=False).get("amdhsa.kernels", []):
                    meta[k[".name"]] = k
        funcs = _functions(elf)
        assert set(meta) <= set(funcs), "a kernel without a function symbol"
        for sym, code in funcs.items():
            out.setdefault(sym, []).append((code, meta.get(sym)))
    for v in out.values():
        v.sort(key=lambda e: e[0])
    return out


def _why(a, b):
    if len(a) != len(b):
        return f"{len(a)} vs {len(b)} definitions"
    why = []
    for (ca, ma), (cb, mb) in zip(a, b):
        if ca != cb:
            why.append(f".text {len(ca)} vs {len(cb)} bytes" if len(ca) != len(cb) else f".text differs ({len(ca)} bytes)")
        if ma != mb:
            keys = sorted(k for k in set(ma or {}) | set(mb or {}) if (ma or {}).get(k) != (mb or {}).get(k))
            why.append("metadata " + ", ".join(f"{k} {(ma or {}).get(k)!r} -> {(mb or {}).get(k)!r}" for k in keys))
    return "; ".join(why)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow-removed", metavar="REGEX", help="symbols only in OLD that match are listed but do not fail")
    args = ap.parse_args()
    old, new = device_code(args.old), device_code(args.new)
    both = sorted(set(old) & set(new))
    differ = [s for s in both if old[s] != new[s]]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    nk = lambda d, syms: sum(1 for s in syms for e in d[s] if e[1] is not None)
    print(f"functions: {len(old)} old, {len(new)} new, {len(both)} in both ({nk(old, both)} kernels), {len(both) - len(differ)} identical")
    for title, syms, src in (("differ", differ, None), ("only in old", only_old, old), ("only in new", only_new, new)):
        print(f"{title}: {len(syms)}")
        for s in syms:
            print(f"  {s}" + (f"    {_why(old[s], new[s])}" if src is None else ""))
    allowed = re.compile(args.allow_removed) if args.allow_removed else None
    unexpected = [s for s in only_old if not (allowed and allowed.search(s))]
    return 1 if differ or only_new or unexpected else 0


if __name__ == "__main__":
    sys.exit(main())
