#!/usr/bin/env python3
"""Compare two builds of the library kernel by kernel (no GPU needed): kernel_diff.py OLD.so NEW.so [--md FILE]

Both libraries' gfx950 code objects are unbundled the way tests/test_isa_properties.py does it; every `pm::` kernel's whole
disassembly (addresses and encodings stripped; the padding behind the kernel's last instruction dropped) and its metadata note
(VGPRs, SGPRs, scratch, LDS) are compared.  The waves-per-SIMD step is taken from `vgpr_count` alone: these kernels use no AGPRs.
A kernel counts as identical when both agree.  For a changed kernel the table gives what decides occupancy and memory-level parallelism: the VGPR
allocation's waves-per-SIMD step, the LDS size, and the 16-byte row loads issued between two full waits (the test module's counter).
Exit status 1 if the symbol sets differ, a forward-family kernel uses scratch, or a changed kernel misses one of the three properties.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FORWARD = ("17embbag_fwd_kernel", "22embbag_fwd_flat_kernel", "14pad_fwd_kernel", "23embbag_fwd_split_kernel")
# the backward's apply kernels: rows of their own in the summary table (reporting only: the pass / fail rule names no family but FORWARD)
BACKWARD = ("22bwd_sorted_main_kernel", "23bwd_sorted_fixup_kernel", "17bwd_unique_kernel", "15hyb_rest_kernel")
# the split forward's private element types became fwd::bf16_t / fwd::f16_t: the same kernels under another type name
RENAMED = {"NS0_7sbf16_tE": "NS_3fwd6bf16_tE", "NS0_6sf16_tE": "NS_3fwd5f16_tE"}

_spec = importlib.util.spec_from_file_location("isa_props", os.path.join(ROOT, "tests", "test_isa_properties.py"))
_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_isa)
row_loads = _isa._row_loads_between_full_waits


def waves_per_simd(vgprs):
    """registers are allocated in granules of 8 per lane; waves per SIMD = min(8, 512 // allocation)"""
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def canonical(name):
    for old, new in RENAMED.items():
        name = name.replace(old, new)
    return name


def kernels(lib, tmp):
    """{mangled name: (instruction lines, (vgprs, sgprs, scratch, lds))} of every pm:: kernel of the library"""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    data = open(fat, "rb").read()
    pos = [m.start() for m in re.finditer(re.escape(MAGIC), data)] + [len(data)]
    out = {}
    for k, (a, b) in enumerate(zip(pos, pos[1:])):
        src, co = os.path.join(tmp, f"s{k}.bin"), os.path.join(tmp, f"s{k}.co")
        open(src, "wb").write(data[a:b])
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + src, "--output=" + co], capture_output=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        meta = {}
        for blk in notes.split("  - .agpr_count")[1:]:
            g = lambda key: re.search(r"\." + key + r":\s+(\S+)", blk).group(1)           # noqa: E731
            meta[g("name")] = (int(g("vgpr_count")), int(g("sgpr_count")), int(g("private_segment_fixed_size")),
                               int(g("group_segment_fixed_size")))
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
            name = m.group(1)
            if not name.startswith("_ZN2pm") or name not in meta:
                continue
            text = [ln.split("//")[0].strip() for ln in m.group(2).splitlines()]
            text = [canonical(ln) for ln in text if ln and not ln.startswith("s_code_end")]
            while text and text[-1].startswith("s_nop"):              # alignment padding behind the kernel
                text.pop()
            key = canonical(name)
            assert key not in out, "two kernels of one name: " + key
            out[key] = (text, meta[name])
        os.remove(src)
        os.remove(co)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", help="write the table of changed kernels here (markdown)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(args.old, tmp), kernels(args.new, tmp)
    bad = []
    if set(old) != set(new):
        bad.append(f"symbol sets differ: only old {sorted(set(old) - set(new))[:5]}, only new {sorted(set(new) - set(old))[:5]}")
    scratch = [n for n, (_t, m) in new.items() if any(f in n for f in FORWARD) and m[2] != 0]
    if scratch:
        bad.append(f"forward kernels with scratch: {scratch[:5]}")
    rows, fam = [], {}
    for n in sorted(set(old) & set(new)):
        (to, mo), (tn, mn) = old[n], new[n]
        family = next((f[2:] for f in FORWARD + BACKWARD if f in n), "other")
        c = fam.setdefault(family, [0, 0])
        if to == tn and mo == mn:
            c[0] += 1
            continue
        c[1] += 1
        lo, ln = row_loads("\n".join(to)), row_loads("\n".join(tn))
        ok = waves_per_simd(mo[0]) == waves_per_simd(mn[0]) and mo[3] == mn[3] and ln >= lo and mn[2] == 0
        if not ok:
            bad.append("changed kernel misses a property: " + n)
        rows.append((n, family, len(to), len(tn), mo[0], mn[0], waves_per_simd(mo[0]), waves_per_simd(mn[0]), mo[3], mn[3], lo, ln, ok))
    lines = ["| family | identical | changed |", "|---|---|---|"]
    lines += [f"| {f} | {c[0]} | {c[1]} |" for f, c in sorted(fam.items())]
    if rows:
        worst = max(rows, key=lambda r: r[3] / r[2])
        lines += ["", f"largest growth in static instructions: {worst[2]} -> {worst[3]} ({100.0 * (worst[3] / worst[2] - 1):+.1f} %), `{worst[0]}`",
                  f"largest VGPR increase: {max(r[5] - r[4] for r in rows):+d}; changed kernels that keep all three properties: "
                  f"{sum(r[12] for r in rows)} of {len(rows)}", "",
                  "| kernel | instructions old -> new | VGPRs old -> new | waves/SIMD | LDS | row loads between full waits | ok |",
                  "|---|---|---|---|---|---|---|"]
        lines += [f"| `{r[0]}` | {r[2]} -> {r[3]} | {r[4]} -> {r[5]} | {r[6]} -> {r[7]} | {r[8]} -> {r[9]} | {r[10]} -> {r[11]} | {'yes' if r[12] else 'NO'} |"
                  for r in rows]
    text = "\n".join(lines) + "\n"
    if args.md:
        open(args.md, "w").write(text)
        print("\n".join(lines[:len(fam) + 6]))
    else:
        print(text)
    for b in bad:
        print("FAIL:", b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
