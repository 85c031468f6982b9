"""Per-kernel comparison of the gfx950 device code of two builds of libdh3d_hip.so.
usage: python tools/device_code_diff.py OLD/libdh3d_hip.so NEW/libdh3d_hip.so  (exit status 1 if anything differs)"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(so):
    """{symbol: sha256 of its disassembled instruction stream (encodings included)} over every gfx950 code object"""
    out, nlines = {}, [0]
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(d, "x.so")])
        blob = open(fat, "rb").read()
        nobj, pos = 0, blob.find(MAGIC)
        while pos >= 0:
            (n,) = struct.unpack_from("<Q", blob, pos + 24)
            p = pos + 32
            for _ in range(n):
                off, size, tl = struct.unpack_from("<QQQ", blob, p)
                triple = blob[p + 24:p + 24 + tl].decode()
                p += 24 + tl
                if "gfx950" not in triple:
                    continue
                co = os.path.join(d, "co%d.o" % nobj)
                nobj += 1
                open(co, "wb").write(blob[pos + off:pos + off + size])
                txt = subprocess.check_output([LLVM + "llvm-objdump", "-d", "--no-leading-addr", co]).decode()
                name = None
                for line in txt.splitlines():
                    m = re.match(r"^<(.+)>:$", line.strip()) or re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
                    if m:
                        name = m.group(1)
                        assert name not in out, name
                        out[name] = hashlib.sha256()
                    elif name and line.strip():
                        out[name].update(line.strip().encode() + b"\n")
                        nlines[0] += 1
            pos = blob.find(MAGIC, pos + 1)
    return {k: v.hexdigest() for k, v in out.items()}, (nobj, nlines[0])


def main(old, new):
    (a, na), (b, nb) = kernels(old), kernels(new)
    print("code objects: %d vs %d; device functions: %d vs %d; instructions: %d vs %d"
          % (na[0], nb[0], len(a), len(b), na[1], nb[1]))
    print("only in old:", sorted(set(a) - set(b)))
    print("only in new:", sorted(set(b) - set(a)))
    diff = sorted(k for k in a if k in b and a[k] != b[k])
    print("instruction streams that differ: %d" % len(diff))
    for k in diff:
        print("  ", k)
    return 1 if diff or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
