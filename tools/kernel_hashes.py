#!/usr/bin/env python3
"""Per-kernel hashes of `hipcc -S --cuda-device-only` output, to show that moving kernels between translation units left
the device code alone.

    kernel_hashes.py a.s [b.s ...]            one line per kernel: symbol, sha256 of its instruction stream and its
                                              .amdhsa_* descriptor lines, the file it came from
    kernel_hashes.py --compare parent.s -- new1.s new2.s ...
                                              every kernel of parent.s must appear exactly once across the new files
                                              with the same hash, and the new files must hold no other kernel; exit 1 if not

What is hashed: the lines between `<symbol>:` and its `.Lfunc_end` -- the instructions, then the `.amdhsa_kernel` block
(registers, LDS, scratch and the rest of the descriptor) -- without comments and blank lines, and with the function number
taken out of local labels (`.LBB12_3` -> `.LBB_3`: it is the function's position in its file).  A reference to a private
constant object that the compiler numbers per module (`.crctable.78@rel32`) is hashed as the object's data."""
import hashlib
import re
import sys

LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)(\d+)(_\d+)?")


PRIVATE_REF = re.compile(r"(\.[A-Za-z_]\w*(?:\.\d+)?)@rel32")


def private_objects(lines):
    """{name: sha256 of its data} of the file's private constant objects (`.crctable.78:` ... `.size .crctable.78, 1024`):
    the compiler numbers them per module, so a kernel's reference to one is hashed as the data it points at"""
    out = {}
    for i, l in enumerate(lines):
        if l.startswith(".") and l.endswith(":") and not l.startswith((".L", ".text")):
            name, h = l[:-1], hashlib.sha256()
            for d in lines[i + 1:]:
                d = d.split(";")[0].strip()
                if d.startswith(".size"):
                    out[name] = h.hexdigest()[:16]
                    break
                h.update((d + "\n").encode())
    return out


def kernels(path):
    """{symbol: sha256} of one assembly file"""
    with open(path) as f:
        lines = f.read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    objects = private_objects(lines)
    out = {}
    for name in names:
        h = hashlib.sha256()
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        descriptor = False
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if not l:
                continue
            descriptor = descriptor or l == ".amdhsa_kernel " + name
            l = LABEL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(3) or ""), l)
            l = PRIVATE_REF.sub(lambda m: "<data %s>@rel32" % objects[m.group(1)] if m.group(1) in objects else m.group(0), l)
            h.update((l + "\n").encode())
        assert descriptor, "%s: no .amdhsa_kernel block inside %s" % (path, name)
        assert name not in out, "%s: %s twice" % (path, name)
        out[name] = h.hexdigest()
    return out


def main(argv):
    if argv and argv[0] == "--compare":
        sep = argv.index("--")
        parent = {}
        for p in argv[1:sep]:
            parent.update(kernels(p))
        seen = {}
        bad = 0
        for p in argv[sep + 1:]:
            for name, digest in kernels(p).items():
                if name in seen:
                    print("TWICE   %s in %s and %s" % (name, seen[name][1], p))
                    bad += 1
                seen[name] = (digest, p)
        for name, digest in sorted(parent.items()):
            if name not in seen:
                print("MISSING %s" % name)
                bad += 1
            elif seen[name][0] != digest:
                print("DIFFERS %s (%s)" % (name, seen[name][1]))
                bad += 1
        for name in sorted(set(seen) - set(parent)):
            print("NEW     %s (%s)" % (name, seen[name][1]))
            bad += 1
        print("%d kernels in the parent, %d in the new files, %d problems" % (len(parent), len(seen), bad))
        return 1 if bad else 0
    for p in argv:
        for name, digest in sorted(kernels(p).items()):
            print("%s  %s  %s" % (digest, name, p.rsplit("/", 1)[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
