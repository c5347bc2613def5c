"""In-tree build of the native library (hipcc, gfx950).  No JIT cache: the ``.so`` lives next
to the sources so that it travels with the repository snapshot to the GPU box.

This module owns the list of translation units and the flags: the product build, the A/B
builds (``tools/build_ab.sh``) and the register report (``tools/kernel_regs.sh``) all take
their compile lines from :func:`command` / :func:`device_commands`, also from the shell:

    python build.py                        build the product library (forced)
    python build.py --out LIB [FLAG ...]   the same sources and flags (+ FLAGs) into LIB
    python build.py --device DIR [FLAG ...]   every .hip TU's device code alone, DIR/<tu>.co
    (``--print`` first: show the compile lines instead of running them)

Provenance: the library embeds ``slgbuild:<digest>`` (``slg_build_id()``), the sha256 of every
file under ``csrc/`` (compiled or included), the public header and the compile flags.
:func:`needs_build` rebuilds whenever the digest of the sources present differs from the one in
the library (content, not mtimes), and ``_native.lib()`` refuses a product library whose digest
does not match them."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
# the compiled files; the headers beside them (DESIGN.md §11 lists them) enter the digest
# through their directory
SRCS = [os.path.join(CSRC, n) for n in ("slgpu.hip", "stats.hip", "ply.hip", "color_gray.hip", "png_device.hip",
                                        "cloud_grid.hip", "cloud_filter.hip", "cloud_cluster.hip",
                                        "cloud_normals.hip", "cloud_icp.hip", "cloud_feature.hip",
                                        "cloud_ransac.hip", "cloud_plane.hip", "cloud_orient.hip", "cloud_mesh.hip", "cloud_meshpost.hip",
                                        "cloud_decimate.hip", "cloud_surface.hip", "cloud_band.hip", "cloud_audit.hip",
                                        "cloud_intersect.hip",
                                        "code_object.cpp",
                                        "png_gray.cpp",
                                        "gather.cpp")]
SRC_SUFFIXES = (".hip", ".cpp", ".h")
HDR = os.path.join(ROOT, "include", "slgpu.h")
HDR_SURFACE = os.path.join(ROOT, "include", "slgpu_surface.h")     # the surface mesher's table (csrc/cloud_surface.hip)
HDR_BAND = os.path.join(ROOT, "include", "slgpu_band.h")           # the banded mesher's table (csrc/cloud_band.hip)
HDR_AUDIT = os.path.join(ROOT, "include", "slgpu_audit.h")         # the mesh audit's table (csrc/cloud_audit.hip)
HDR_INTERSECT = os.path.join(ROOT, "include", "slgpu_intersect.h")   # the self-intersection test's table (csrc/cloud_intersect.hip)
OUT = os.path.join(PKG, "libslgpu.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-sched-strategy=max-ilp: the machine scheduler interleaves main3's independent fp64
# chains and loads more aggressively (243.8 vs 246.1 us per 12-view launch, bit-identical output,
# profiles/r3af); max-memory-clause was 1 % and iterative-minreg 5 % slower (profiles/r3ae)
COMPILE_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-mllvm",
                 "-amdgpu-sched-strategy=max-ilp"]
FLAGS = [*COMPILE_FLAGS, "-fPIC", "-shared"]
LIBS = ["-lz", "-ldl"]
BUILD_ID_PREFIX = b"slgbuild:"


def command(out: str, extra_flags=()) -> list[str]:
    """The compile line of the whole library into ``out``: FLAGS, ``extra_flags``, every TU."""
    return [HIPCC, *FLAGS, *extra_flags, "-o", out, *SRCS, *LIBS]


def device_commands(out_dir: str, extra_flags=()) -> list[list[str]]:
    """One compile line per ``.hip`` TU: its device code alone (an offload bundle) into
    ``out_dir/<tu>.co``, with the product's compile flags."""
    return [[HIPCC, *COMPILE_FLAGS, "--cuda-device-only", *extra_flags, "-c", p, "-o",
             os.path.join(out_dir, os.path.splitext(os.path.basename(p))[0] + ".co")]
            for p in SRCS if p.endswith(".hip")]


def digest_files(srcs=None) -> list[str]:
    """What the digest reads: the compiled files, every source or header beside them, and the
    public headers."""
    srcs = list(srcs or SRCS)
    beside = {os.path.join(d, n) for d in {os.path.dirname(p) for p in srcs} for n in os.listdir(d)
              if n.endswith(SRC_SUFFIXES)}
    # by name, as the digest names them; the surface, band, audit and intersect tables are included by their units like
    # the headers beside them, so a copy of one beside copied sources stands for it
    by_name = {os.path.basename(p): p for p in (HDR_SURFACE, HDR_BAND, HDR_AUDIT, HDR_INTERSECT, *sorted(beside.union(srcs)))}
    return [*(by_name[k] for k in sorted(by_name)), HDR]


def source_digest(srcs=None, flags=None) -> str:
    """sha256 (32 hex digits) of :func:`digest_files` (name + bytes) and the flags."""
    h = hashlib.sha256()
    for p in digest_files(srcs):
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update("\0".join(flags or FLAGS).encode())
    return h.hexdigest()[:32]


def built_digest(path: str = OUT) -> str | None:
    """The digest embedded in a built library (read from the file; nothing is loaded)."""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    m = re.search(re.escape(BUILD_ID_PREFIX) + rb"([0-9a-f]{32})", data)
    return m.group(1).decode() if m else None


def needs_build() -> bool:
    return built_digest() != source_digest()


def build_native(force: bool = False, verbose: bool = False) -> str:
    """Compile every TU of ``csrc/`` into ``libslgpu.so`` (skipped when the embedded digest
    matches the sources)."""
    if force or needs_build():
        digest = source_digest()
        cmd = command(OUT + ".tmp", [f'-DSLG_BUILD_ID="{BUILD_ID_PREFIX.decode()}{digest}"'])
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(OUT + ".tmp", OUT)
        if verbose:
            print(f"built {OUT} for gfx950 (build id {digest})")
    elif verbose:
        print(f"{OUT} matches its sources (build id {built_digest()}): not rebuilt")
    return OUT


def main(argv: list[str]) -> None:
    show = argv[:1] == ["--print"]
    argv = argv[1:] if show else argv
    if not argv:
        cmds = None if not show else [command(OUT, ['-DSLG_BUILD_ID="..."'])]
    elif argv[0] == "--out" and len(argv) > 1:
        cmds = [command(argv[1], argv[2:])]
    elif argv[0] == "--device" and len(argv) > 1:
        cmds = device_commands(argv[1], argv[2:])
    else:
        raise SystemExit(__doc__)
    if cmds is None:
        print(build_native(force=True, verbose=True))
    elif show:
        print("\n".join(" ".join(cmd) for cmd in cmds))
    else:                                      # (the TUs of --device compile side by side)
        if any([p.wait() for p in [subprocess.Popen(cmd) for cmd in cmds]]):
            raise SystemExit(1)


if __name__ == "__main__":
    main(sys.argv[1:])
