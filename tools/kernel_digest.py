#!/usr/bin/env python3
"""Digest of every kernel's machine code, to answer "did this edit change any kernel?" without a GPU.

    python tools/kernel_digest.py build OUT.json [-DNAME ...]   compile every source device-only and write the digests
    python tools/kernel_digest.py diff A.json B.json            print what appeared, vanished or differs; exit 1 if anything does
                                                                (a vanished and an appeared kernel with equal records: "renamed", no difference)

``build`` compiles each of ``_native.SOURCES`` with ``_native.HIPCC_FLAGS`` plus ``--cuda-device-only
--no-gpu-bundle-output -c`` into a scratch directory, which yields one plain elf64-amdgpu object per source, and records
for every kernel, keyed by mangled name: the SHA-256 of its ``.text`` bytes, its 64-byte ``.kd`` descriptor (without the
code entry offset, which only says where in the object the linker put the code), and the register, scratch, LDS and
kernel-argument sizes of the object's metadata note.  It hashes and compares; it does not look at the instructions.  The
kernels live in unnamed namespaces, so a kernel keeps its name when it moves to another file.  A kernel that addresses a
``__device__`` variable (k_c2f_pair32 and g_zero_line) holds the distance to it in its code, so its hash changes whenever
the object's layout does; compare such a kernel's ``llvm-objdump -d --no-show-raw-insn`` text instead.  A template that loses a
parameter renames its instantiations: ``diff`` pairs a vanished kernel with an appeared one when their records are equal in every
field but ``source`` and exactly one candidate exists on either side, and prints the pair as renamed.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from realtime_video_analytics_32streams_amd import _native as N  # noqa: E402

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def _run(*cmd) -> str:
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, text=True).stdout


def _digest_object(obj: Path, source: str) -> dict:
    """{mangled name: digest record} of one elf64-amdgpu object."""
    blob = obj.read_bytes()
    sections = {}                                    # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", _run(LLVM / "llvm-readelf", "-S", "-W", obj), re.M):
        sections[int(m[1])] = (int(m[2], 16), int(m[3], 16))
    syms = {}                                        # name -> bytes, from .symtab (it repeats .dynsym)
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", _run(LLVM / "llvm-readelf", "-s", "-W", obj), re.M):
        addr, off = sections[int(m[4])]
        at = off + int(m[1], 16) - addr
        syms[m[5]] = blob[at:at + int(m[2])]
    out, cur = {}, None
    for line in _run(LLVM / "llvm-readelf", "--notes", obj).splitlines():
        if line.startswith("  - "):                  # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.\w+):\s*(\S+)$", line)
        if cur is None or not m:
            continue
        if m[1] == ".name":
            out[m[2]] = cur
        elif m[1] in META:
            cur[m[1]] = int(m[2])
    for name, rec in out.items():
        kd = syms[name + ".kd"]
        assert len(kd) == 64 and len(syms[name]) > 0 and set(rec) == set(META), f"{obj.name}: incomplete record for {name}"
        kd = kd[:16] + bytes(8) + kd[24:]            # kernel_code_entry_byte_offset: where the linker put the code, not what it is
        rec.update(source=source, text_size=len(syms[name]), text_sha256=hashlib.sha256(syms[name]).hexdigest(), kd=kd.hex())
    return out


def build(out_json: str, defines: list) -> int:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        def one(src):
            obj = Path(tmp) / (src + ".o")
            subprocess.run([hipcc, *N.HIPCC_FLAGS, *defines, f"-I{N.ROOT / 'include'}", "--cuda-device-only", "--no-gpu-bundle-output",
                            "-Wno-unused-command-line-argument", "-c", str(N.CSRC / src), "-o", str(obj)], check=True, cwd=str(N.CSRC))
            return _digest_object(obj, src)
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(one, N.SOURCES))
    kernels = {}
    for part in parts:
        for name, rec in part.items():
            assert name not in kernels, f"{name} is defined in {kernels[name]['source']} and in {rec['source']}"
            kernels[name] = rec
    Path(out_json).write_text(json.dumps({"flags": N.HIPCC_FLAGS + defines, "kernels": kernels}, indent=1, sort_keys=True) + "\n")
    print(f"{len(kernels)} kernels from {len(N.SOURCES)} sources -> {out_json}")
    return 0


def _by_record(kernels: dict, names) -> dict:
    """{a record without its ``source``, as text: the names among ``names`` that carry it}"""
    out = {}
    for name in sorted(names):
        out.setdefault(json.dumps({k: v for k, v in kernels[name].items() if k != "source"}, sort_keys=True), []).append(name)
    return out


def diff(a_json: str, b_json: str) -> int:
    a, b = (json.loads(Path(p).read_text())["kernels"] for p in (a_json, b_json))
    bad = 0
    gone, new = _by_record(a, set(a) - set(b)), _by_record(b, set(b) - set(a))
    renamed = {v[0]: new[k][0] for k, v in gone.items() if len(v) == 1 and len(new.get(k, ())) == 1}
    for old, name in sorted(renamed.items()):
        print(f"renamed: {old} -> {name}")
    for name in sorted(set(a) | set(b)):
        if name in renamed or name in renamed.values():
            continue
        if name not in b or name not in a:
            print(f"{'vanished' if name in a else 'appeared'}: {name}")
            bad += 1
            continue
        keys = [k for k in sorted(set(a[name]) | set(b[name])) if k != "source" and a[name].get(k) != b[name].get(k)]
        if keys:
            print(f"differs: {name}: " + ", ".join(f"{k} {a[name].get(k)} -> {b[name].get(k)}" if k in META or k == "text_size" else k for k in keys))
            bad += 1
    moved = sum(1 for n in a if n in b and a[n]["source"] != b[n]["source"])
    print(f"{len(a)} kernels before, {len(b)} after, {moved} in another source, {len(renamed)} renamed, {bad} appeared, vanished or differing")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "build":
        sys.exit(build(sys.argv[2], sys.argv[3:]))
    if len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
