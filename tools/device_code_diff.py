#!/usr/bin/env python3
"""(host) Is the device code of two builds of the library the same?   python tools/device_code_diff.py A.so B.so [A_KERNEL=B_KERNEL ...]

Unbundles both with `llvm-objdump --offloading` and compares, per gfx950 code object (one per .hip file, in link order), the set
of kernels and the bytes of .text and .rodata (the kernel descriptors live there). Where a whole section differs -- e.g. the
same kernels emitted in another order -- every kernel is compared on its own: the function's bytes and its 64-byte descriptor
`<kernel>.kd` (without its entry offset, which moves when a kernel is added); the ones that differ are printed. A_KERNEL=B_KERNEL (mangled names) compares a kernel of A with the kernel of B that took its place
under another name, e.g. one that became the instantiation of a template; kernels only B has are then listed, not counted. Exit
status 0 only if everything else matches. What a host-side refactor has to show."""
import glob
import os
import shutil
import struct
import subprocess
import sys
import tempfile


def code_objects(lib, tmp):
    """The gfx950 code objects of `lib` as bytes, in bundle order (llvm-objdump writes them next to the file it reads)."""
    objdump = shutil.which("llvm-objdump") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump")
    os.makedirs(tmp)
    copy = shutil.copy(lib, tmp)
    subprocess.check_call([objdump, "--offloading", os.path.basename(copy)], cwd=tmp, stdout=subprocess.DEVNULL)
    found = glob.glob(copy + ".*gfx950*")
    return [open(f, "rb").read() for f in sorted(found, key=lambda f: int(f[len(copy) + 1:].split(".")[0]))]


def parse(elf):
    """(sections {name: (addr, bytes)}, symbols {name: (section name, value, size)}) of a little-endian ELF64 image."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    cstr = lambda table, at: table[at:table.index(b"\0", at)].decode()
    body = lambda h: b"" if h[1] == 8 else elf[h[4]:h[4] + h[5]]            # SHT_NOBITS holds no bytes
    names = [cstr(body(heads[shstrndx]), h[0]) for h in heads]
    sections = {n: (h[3], body(h)) for n, h in zip(names, heads)}
    symbols = {}
    symtab = next(h for h in heads if h[1] == 2)                               # SHT_SYMTAB; its sh_link is the string table
    strtab = body(heads[symtab[6]])
    for at in range(0, symtab[5], 24):
        name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", body(symtab), at)
        if 0 < shndx < shnum:
            symbols[cstr(strtab, name)] = (names[shndx], value, size)
    return sections, symbols


def symbol_bytes(sections, symbols, name):
    sec, value, size = symbols[name]
    addr, data = sections[sec]
    return data[value - addr:value - addr + size]


# kernel_descriptor_t (llvm AMDGPUUsage, "Kernel Descriptor"): bytes 16..24 are KERNEL_CODE_ENTRY_BYTE_OFFSET, the distance from the
# descriptor to the kernel's first instruction
KD_ENTRY_OFFSET = slice(16, 24)


def without_entry_offset(kd):
    return kd[:KD_ENTRY_OFFSET.start] + kd[KD_ENTRY_OFFSET.stop:]


def main(a, b, renamed=()):
    to_b = dict(pair.split("=") for pair in renamed)
    with tempfile.TemporaryDirectory() as tmp:
        objs_a, objs_b = code_objects(a, os.path.join(tmp, "a")), code_objects(b, os.path.join(tmp, "b"))
    same = len(objs_a) == len(objs_b) and len(objs_a) > 0
    print("%s: %d gfx950 code objects; %s: %d" % (a, len(objs_a), b, len(objs_b)))
    for i, (ea, eb) in enumerate(zip(objs_a, objs_b)):
        (sec_a, sym_a), (sec_b, sym_b) = parse(ea), parse(eb)
        kern_a, kern_b = ({s[:-3] for s in sym if s.endswith(".kd")} for sym in (sym_a, sym_b))
        whole = {s: sec_a.get(s, (0, b""))[1] == sec_b.get(s, (0, b""))[1] for s in (".text", ".rodata")}
        print("code object %d: %d kernels; " % (i, len(kern_a)) + "; ".join(
            "%s %d bytes %s" % (s, len(sec_a.get(s, (0, b""))[1]), "identical" if ok else "DIFFERS") for s, ok in whole.items()))
        here = {k: v for k, v in to_b.items() if k in kern_a and v in kern_b}
        if here:
            print("  compared under another name: " + ", ".join("%s = %s" % kv for kv in sorted(here.items())))
            if kern_b - set(here.values()) - kern_a:
                print("  kernels only in %s: %s" % (b, sorted(kern_b - set(here.values()) - kern_a)))
            kern_b = (kern_b - set(here.values())) & kern_a | set(here)
            sym_b = dict(sym_b, **{k + tail: sym_b[v + tail] for k, v in here.items() for tail in ("", ".kd")})
        if kern_a != kern_b:
            same = False
            print("  kernels only in %s: %s\n  kernels only in %s: %s" % (a, sorted(kern_a - kern_b), b, sorted(kern_b - kern_a)))
        if not all(whole.values()) or here:
            # a descriptor holds the offset from itself to the kernel's entry (KD_ENTRY_OFFSET), which moves with every kernel added
            # to or taken from the code object: compared with that field left out, and reported apart from the function's bytes
            def parts(k):
                kd_a, kd_b = symbol_bytes(sec_a, sym_a, k + ".kd"), symbol_bytes(sec_b, sym_b, k + ".kd")
                out = [] if symbol_bytes(sec_a, sym_a, k) == symbol_bytes(sec_b, sym_b, k) else ["function bytes"]
                if without_entry_offset(kd_a) != without_entry_offset(kd_b):
                    out.append("descriptor")
                return out, kd_a != kd_b
            report = {k: parts(k) for k in sorted(kern_a & kern_b)}
            differ = [k for k, (what, _) in report.items() if what]
            moved = [k for k, (what, kd) in report.items() if kd and not what]
            print("  per kernel (function bytes + descriptor): %d of %d differ" % (len(differ), len(report)))
            for k in differ:
                same = False
                print("    %s: %s" % (k, ", ".join(report[k][0])))
            if moved:
                print("  identical but for the descriptor's entry offset (the kernel sits elsewhere in .text): %d" % len(moved))
                for k in moved:
                    print("    " + k)
    print("device code: " + ("IDENTICAL" if same else "DIFFERENT"))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) < 3 or not all("=" in pair for pair in sys.argv[3:]):
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
