"""Resource usage and code size of every kernel of two builds of libpcbenv.so, side by side.
python tools/kernel_resource_diff.py OLD_OBJDIR NEW_OBJDIR

The object directories are what build.py leaves under build/<library name>/.  Per translation unit, the gfx950 code object
is unbundled from the .hip_fatbin section of the unit's object file; a kernel's registers, spills, scratch and static LDS
are its entry in the code object's metadata note -- the figures `-Rpass-analysis=kernel-resource-usage` prints, read per
unit instead of from the interleaved output of a parallel build -- its code size is the size of its symbol and its code
digest a hash of that symbol's bytes in .text (the instructions themselves: two builds with equal digests run the same
code, whatever else in the files differs).  Prints
one line per (unit, kernel) that exists only in OLD or differs, the kernels only NEW has in full, and a summary; exit
status 1 if anything of OLD's is missing or different."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")


def kernels(objdir):
    """{(unit, kernel symbol): {field: value}} over the units with device code."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(objdir)):
            if not f.endswith(".hip.o"):
                continue
            unit = f[:-len(".hip.o")]
            fb, co = os.path.join(tmp, f + ".fatbin"), os.path.join(tmp, f + ".co")
            if subprocess.call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, os.path.join(objdir, f)],
                               stderr=subprocess.DEVNULL) != 0:
                continue  # a unit without device code
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co])
            cur = {}
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True).splitlines():
                if line.lstrip().startswith("- .agpr_count"):  # the first key of a kernel's entry
                    cur = {}
                m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)\s*$", line)
                if not m:
                    continue
                if m.group(1) in FIELDS:
                    cur[m.group(1)] = m.group(2)
                elif m.group(1) == ".name":
                    out[(unit, m.group(2))] = cur
            text = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)",
                             subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-SW", co], text=True))
            addr, off = int(text.group(1), 16), int(text.group(2), 16)
            image = open(co, "rb").read()
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", co], text=True).splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND" and (unit, p[7]) in out:
                    out[(unit, p[7])]["code_bytes"] = p[2]
                    start = off + int(p[1], 16) - addr
                    assert addr <= int(p[1], 16) and start + int(p[2]) <= off + int(text.group(3), 16), (unit, p[7])
                    out[(unit, p[7])]["code_digest"] = hashlib.sha256(image[start:start + int(p[2])]).hexdigest()[:16]
    return out


def demangle(name):
    try:
        return subprocess.check_output(["c++filt", name], text=True).strip().split("(")[0].replace("void ", "")
    except (OSError, subprocess.CalledProcessError):
        return name


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    cols = FIELDS + ("code_bytes", "code_digest")
    moved = 0
    for key in sorted(old):
        if key not in new:
            print("only in OLD:", *key)
            moved += 1
        elif old[key] != new[key]:
            moved += 1
            print("DIFFERS:", *key, {c: (old[key].get(c), new[key].get(c)) for c in cols if old[key].get(c) != new[key].get(c)})
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {len(set(old) & set(new))} in both; {moved} of OLD's missing or different "
          f"in any of {', '.join(c.lstrip('.') for c in cols)}")
    fresh = sorted(set(new) - set(old))
    if fresh:
        print("only in NEW (unit: kernel: " + " | ".join(c.lstrip(".") for c in cols) + "):")
        for key in fresh:
            print(f"  {key[0]}: {demangle(key[1])}: " + " | ".join(new[key].get(c, "?") for c in cols))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
