#!/usr/bin/env python3
"""Register / scratch / LDS use of every kernel in libmf_hip.so, read from the code objects' notes.

hipcc embeds one clang offload bundle per translation unit in the ``.hip_fatbin`` section; each bundle holds the gfx950
code object whose ``NT_AMDGPU_METADATA`` note lists, per kernel, ``.vgpr_count``, ``.agpr_count``, ``.sgpr_count``,
``.vgpr_spill_count``, ``.sgpr_spill_count``, ``.private_segment_fixed_size`` (scratch bytes per lane) and
``.group_segment_fixed_size`` (static LDS).  No GPU needed: ``tests/test_host_cpu.py`` asserts from this that no kernel
of the product paths spills.

    python tools/kernel_resources.py [path/to/libmf_hip.so] [--spills]
    python tools/kernel_resources.py [path/to/libmf_hip.so] --text-digest [--only=update_fused,update_rows]   # JSON

``--text-digest``: beside the figures, one sha256 of each kernel's disassembled instruction text -- to show that a refactor
left the generated code of a kernel as it was (compare two builds' outputs).  ``--names-of=record.json`` keeps only the kernels
an earlier record names: a branch that adds kernels beside the old ones gives a record to compare with the parent's as it is.
"""
from __future__ import annotations

import hashlib
import json
import pathlib
import re
import struct
import subprocess
import sys
import tempfile

LLVM = pathlib.Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = pathlib.Path(__file__).resolve().parents[1]
DEFAULT_LIB = ROOT / "matrix-factorization-torch_amd" / "lib" / "libmf_hip.so"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size", "max_flat_workgroup_size")


def code_objects(lib: pathlib.Path) -> list[bytes]:
    """The gfx950 code objects of every bundle in the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as tmp:
        fat = pathlib.Path(tmp) / "fat.bin"
        subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
        data = fat.read_bytes()
    out = []
    for m in re.finditer(re.escape(MAGIC), data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24: pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[base + off: base + off + size])
    return out


def demangle(names: list[str]) -> list[str]:
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        out = res.stdout.splitlines()
        return out if len(out) == len(names) else names
    except (OSError, subprocess.CalledProcessError):
        return names


def kernel_resources(lib: pathlib.Path = DEFAULT_LIB) -> dict[str, dict[str, int]]:
    """{demangled kernel name: {field: value}} for every kernel of the library."""
    table: dict[str, dict[str, int]] = {}
    for co in code_objects(pathlib.Path(lib)):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", f.name], capture_output=True, text=True, check=True).stdout
        # one YAML map per kernel under amdhsa.kernels: entries start with "  - .agpr_count:" (keys sorted) -- split on list items
        body = notes.split("amdhsa.kernels:", 1)[1] if "amdhsa.kernels:" in notes else ""
        body = body.split("amdhsa.target:", 1)[0]
        for item in re.split(r"\n  - ", "\n" + body)[1:]:
            name = re.search(r"\.name:\s+(\S+)", item)
            if not name:
                continue
            rec = {}
            for fld in FIELDS:
                mm = re.search(rf"\.{fld}:\s+(\d+)", item)
                rec[fld] = int(mm.group(1)) if mm else 0
            table[name.group(1)] = rec
    names = list(table)
    return dict(zip(demangle(names), table.values()))


def text_digests(lib: pathlib.Path = DEFAULT_LIB) -> dict[str, str]:
    """{demangled function name: sha256 of its disassembled instruction text} for every function of the library's code
    objects.  The text is what ``llvm-objdump -d`` prints without addresses and encodings, comments dropped and the
    function's own symbol replaced by a fixed word: two builds whose kernels differ in name only (a template argument that
    changed its type) give the same digests, and so do two builds that lay the same kernel out at another place in the
    code object (the ``s_nop`` padding behind a function's last instruction is dropped).  Nothing else is searched for."""
    table: dict[str, str] = {}
    for co in code_objects(pathlib.Path(lib)):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", f.name],
                                 capture_output=True, text=True, check=True).stdout
        name, lines = None, []
        for line in dis.splitlines() + ["<end>:"]:
            label = re.fullmatch(r"(?:[0-9a-f]+ )?<(\S+)>:", line.strip())
            if label:
                if name is not None:
                    while lines and lines[-1] in ("", "s_nop 0", "..."):     # padding up to the next function's alignment: layout, not code
                        lines.pop()
                    text = "\n".join(x for x in lines if x).replace(name, "SELF")
                    table[name] = hashlib.sha256(text.encode()).hexdigest()
                name, lines = label.group(1), []
            elif name is not None:
                lines.append(line.split("//")[0].strip())
    names = list(table)
    return dict(zip(demangle(names), table.values()))


def main() -> None:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--text-digest" in sys.argv:     # JSON: {kernel: {"text_sha256": ..., the resource figures}}, kernels whose name has one of --only=a,b,..
        lib = pathlib.Path(args[0]) if args else DEFAULT_LIB
        only = next((a.split("=", 1)[1].split(",") for a in sys.argv if a.startswith("--only=")), [""])
        names = next((set(json.loads(pathlib.Path(a.split("=", 1)[1]).read_text())) for a in sys.argv if a.startswith("--names-of=")), None)
        res, dig = kernel_resources(lib), text_digests(lib)
        print(json.dumps({k: {"text_sha256": dig.get(k), **{f: v for f, v in r.items() if f != "max_flat_workgroup_size"}}
                          for k, r in sorted(res.items()) if any(o in k for o in only) and (names is None or k in names)}, indent=1))
        return
    res = kernel_resources(pathlib.Path(args[0]) if args else DEFAULT_LIB)
    only_spills = "--spills" in sys.argv
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'vspill':>6} {'sspill':>6} {'scratch':>7} {'lds':>7}  kernel")
    for name, r in sorted(res.items()):
        if only_spills and not (r["vgpr_spill_count"] or r["private_segment_fixed_size"]):
            continue
        print(f"{r['vgpr_count']:5d} {r['agpr_count']:5d} {r['sgpr_count']:5d} {r['vgpr_spill_count']:6d} {r['sgpr_spill_count']:6d} "
              f"{r['private_segment_fixed_size']:7d} {r['group_segment_fixed_size']:7d}  {name[:150]}")


if __name__ == "__main__":
    main()
