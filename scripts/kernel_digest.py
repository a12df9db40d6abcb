#!/usr/bin/env python
"""Per-kernel digest of two device code objects: kernel_digest.py PARENT.co NEW.co  (exit 1 on any mismatch).

Each object is a device-only, unbundled compile (hipcc ... --cuda-device-only --no-gpu-bundle-output -c).  Every
function symbol's instruction-encoding words (llvm-objdump -d) are hashed; a kernel of NEW passes when PARENT has the
same bytes under the same name or -- a template that lost parameters -- under a name NEW no longer has (the map is
printed).  Kernels only in PARENT are listed as dropped.  A pruning change is behaviour-neutral when nothing fails.
"""
import hashlib
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def digests(path):
    out, name = {}, None
    for line in subprocess.run([OBJDUMP, "-d", "-C", path], check=True, capture_output=True, text=True).stdout.splitlines():
        if m := re.match(r"[0-9a-f]+ <(?:void )?([^(]+).*>:$", line):   # demangled, without the argument list
            name = m.group(1)
            out[name] = [0, hashlib.sha256()]
        elif name and (m := re.search(r"// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)", line)):
            words = bytes.fromhex(m.group(1).replace(" ", ""))
            out[name][0] += len(words)
            out[name][1].update(words)
    return {k: (n, h.hexdigest()[:16]) for k, (n, h) in out.items()}


old, new = digests(sys.argv[1]), digests(sys.argv[2])
free = {h: k for k, (_, h) in old.items() if k not in new}   # parent kernels whose name is gone, by hash
bad = 0
print(f"# parent {len(old)} kernels, new {len(new)} kernels\n# kernel  bytes  sha256[:16]  parent sha256[:16]  (parent name)")
for k, (n, h) in sorted(new.items()):
    was = k if k in old else free.get(h)
    ph = old[was][1] if was else "-"
    bad += ph != h
    print(f"{k}  {n}  {h}  {ph}  {'SAME' if ph == h else 'DIFFERS'}" + (f"  (was {was})" if was and was != k else ""))
gone = sorted(k for k in old if k not in new and k not in [free.get(h) for _, h in new.values()])
print(f"# dropped from the parent ({len(gone)}):", *gone, sep="\n#   ")
print(f"# {len(new) - bad} of {len(new)} kernels identical to the parent's")
sys.exit(1 if bad else 0)
