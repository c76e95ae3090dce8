#!/usr/bin/env python3
"""Digest of the gfx950 device code in HIP object files, kernel by kernel (CPU only: needs the ROCm LLVM tools, no GPU).

usage: tools/device_code_digest.py gato_python_amd/csrc/gato_pcg_*.o > branch.txt    (then diff against the parent's)

Per code symbol (kernel) one line: unit, symbol, SHA-256 (16 hex digits) of its disassembled instructions - leading addresses and the
trailing `// address: encoding` comments stripped, so that a kernel's position in its unit does not matter - and the metadata
that decides occupancy: VGPRs, SGPRs, LDS bytes, scratch bytes, spilled SGPRs / VGPRs.  Per unit one `==` line with the kernel
count and a hash over its kernel lines.  A refactor that must not change device code passes when the two outputs are equal."""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count",
        ".vgpr_spill_count")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def digest(obj, tmp):
    fat, co = os.path.join(tmp, "unit.fat"), os.path.join(tmp, "unit.co")
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj)
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
        "--output=" + co)
    code, name = {}, None                                    # symbol -> instruction lines
    for line in run("llvm-objdump", "-d", co).splitlines():
        label = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if label:
            name = label.group(1)
            code[name] = []
        elif name and line.strip() not in ("", "..."):       # "...": zero padding up to the next symbol
            code[name].append(re.sub(r"\s*//.*$", "", line).strip())
    meta, entry, col = {}, None, None                        # kernel -> its metadata fields (the nested ones of its arguments skipped)
    for line in run("llvm-readelf", "--notes", co).splitlines():
        field = re.match(r"(\s*)(- )?(\.\w+):\s+(\S+)\s*$", line)
        at = field and len(field.group(1)) + (2 if field.group(2) else 0)
        col = at if col is None and field else col           # the first field of all is a kernel's
        if not field or at != col:
            continue
        entry = {} if field.group(2) else entry
        entry[field.group(3)] = field.group(4)
        if field.group(3) == ".name":
            meta[field.group(4)] = entry
    unit = os.path.basename(obj)
    # every code symbol is listed; one that is not a kernel (a device function left out of line) has no metadata
    lines = ["%s %s %s %s" % (unit, k, sha("\n".join(code[k])), " ".join(meta.get(k, {}).get(f, "-") for f in META)) for k in sorted(code)]
    return lines + ["== %s kernels=%d digest=%s" % (unit, len(lines), sha("\n".join(lines)))]


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sys.argv[1:]:
            print("\n".join(digest(obj, tmp)))
