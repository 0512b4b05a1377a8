#!/usr/bin/env python3
"""The registers of the JPEG decoder's kernels in two checkouts, from the code objects' metadata (a tool, not a test; no GPU).

    python tools/jpeg_decode_resources.py PARENT_TREE [--out profiles/jpeg_decode_scale.txt]

Compiles librectify_amd/csrc/kernels_jpeg_decode.hip of PARENT_TREE (a checkout of the parent commit) and of this tree for
gfx950 with the build's flags, keeps the assembly, and reads .vgpr_count, .sgpr_count, .group_segment_fixed_size (LDS) and
.private_segment_fixed_size (scratch) of every kernel from its amdhsa.kernels metadata.  A kernel of this tree stands beside
the parent's kernel of the same name, or, where this tree's templates have one argument more than the parent's (kScaled
of the transform and the output pass), of that name with the new argument false: those are the kernels a call without the new
option launches, and their four numbers must be the parent's.  Exits 1 if they are not.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from librectify_amd import build  # noqa: E402

FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def resources(tree):
    """{demangled kernel name: (VGPRs, SGPRs, LDS bytes, scratch bytes)}"""
    src = os.path.join(tree, "librectify_amd", "csrc", "kernels_jpeg_decode.hip")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([build._hipcc()] + build.FLAGS + ["-x", "hip", "-c", src, "-o", os.path.join(tmp, "d.o"), "-save-temps=obj"])
        asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "amdgcn" in f]
        with open(os.path.join(tmp, asm[0])) as f:
            text = f.read()
    out = {}
    for entry in re.split(r"\n  - \.agpr_count", text)[1:]:
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, entry).group(1)  # noqa: E731
        name = subprocess.run(["c++filt", get("name")], capture_output=True, text=True, check=True).stdout.strip()
        name = re.sub(r"^(void )?lramd::\(anonymous namespace\)::", "", name)
        name = re.sub(r"\((?!lr_pixel_format\)).*", "", name).replace("(lr_pixel_format)", "")
        out[name] = tuple(int(get(k)) for k in FIELDS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_scale.txt"))
    a = ap.parse_args()
    old, new = resources(a.parent_tree), resources(ROOT)
    lines = ["", "== registers of the decoder's kernels, gfx950, from the code objects' metadata: VGPRs / SGPRs / LDS bytes / scratch bytes ==",
             "   (left: the parent commit; right: this commit, the same instantiation, which a call without the new option launches;",
             "    further right the instantiation that a call with LR_JPEG_SCALED and a frame of scale 2, 4 or 8 launches in its place)"]
    same = True
    for name, was in sorted(old.items()):
        special = name if name in new else (name.replace(">", ", false>") if "<" in name else name + "<false>")
        # (the scaled instantiations take the general geometry: kAny and kScaled both true)
        general = re.sub(r"(true|false), false>$", "true, true>", special) if special != name else None
        now = new.get(special)
        same = same and now == was
        fmt = lambda r: "%3d / %3d / %5d / %d" % r if r else "(none)"  # noqa: E731
        lines.append("      %-28s %-24s %-24s %-10s %s" % (name, fmt(was), fmt(now), "equal" if now == was else "DIFFERENT", fmt(new.get(general)) if general else "(the same kernel)"))
    lines.append("   every kernel of a call without the bit has the parent's numbers: %s" % ("yes" if same else "NO"))
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
