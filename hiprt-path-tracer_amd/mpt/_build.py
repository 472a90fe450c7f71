"""Builds libmpt.so (the HIP path tracer + C ABI) in-tree for gfx950.

Plain hipcc invocations, compiled in parallel, relinked only when a source or
header is newer than the library.  Used by ``__graft_entry__.build()`` and by the
test-suite; never invoked implicitly by the product path (``mpt.lib()`` fails
loudly when the library is missing).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
ROOT = PKG_DIR.parent
CSRC = ROOT / "csrc"
INCLUDE = ROOT.parent / "include"
LIB_PATH = PKG_DIR / "libmpt.so"
OBJ_DIR = CSRC / "build"

SOURCES = ["bvh8.cpp", "mpt_kernels.hip", "bake.hip", "mpt_api.cpp", "mpt_geometry.cpp", "image.cpp", "jpeg.cpp", "display.hip", "denoise.hip", "refit.hip", "lbvh.hip", "ploc.hip", "sah.hip", "upload.hip", "xform.hip", "skin.hip", "morph.hip", "anim.hip", "normals.hip", "temporal.hip"]
# mpt_part.hip is compiled once per part (-DMPT_TU_PART=k): the shading and ReSTIR DI kernel
# instantiations, so that they compile in parallel with the rest
PARTS = [1, 2, 3, 4, 5, 6, 7]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
CXXFLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
    "-Wno-unused-result", "-Wno-unused-value", f"-I{INCLUDE}", f"-I{CSRC}",
]


def _deps() -> list[Path]:
    return [CSRC / s for s in SOURCES] + [CSRC / "mpt_part.hip"] + sorted(CSRC.glob("*.h")) + sorted(INCLUDE.glob("*.h"))


def up_to_date() -> bool:
    if not LIB_PATH.exists():
        return False
    t = LIB_PATH.stat().st_mtime
    return all(p.stat().st_mtime <= t for p in _deps())


def build(force: bool = False, verbose: bool = True, defines=(), out: Path | None = None) -> Path:
    """defines/out: development variants (e.g. -DMPT_SHADE_WAVES=2 into another path)."""
    lib_path = Path(out) if out else LIB_PATH
    if not force and not defines and out is None and up_to_date():
        return LIB_PATH
    obj_dir = OBJ_DIR if out is None else lib_path.parent / "obj"
    obj_dir.mkdir(parents=True, exist_ok=True)
    procs = []
    objs = []
    units = [(s, [], Path(s).stem) for s in SOURCES] + [("mpt_part.hip", [f"-DMPT_TU_PART={k}"], f"mpt_part{k}") for k in PARTS]
    for s, extra, stem in units:
        obj = obj_dir / (stem + ".o")
        objs.append(obj)
        cmd = [HIPCC, *CXXFLAGS, *defines, *extra, "-c", str(CSRC / s), "-o", str(obj)]
        if verbose:
            print("[mpt build]", " ".join(cmd), file=sys.stderr)
        procs.append((stem, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    errors = []
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            errors.append(f"{s}:\n{out.decode(errors='replace')}")
    if errors:
        raise RuntimeError("libmpt build failed:\n" + "\n".join(errors))
    tmp = lib_path.with_suffix(".so.tmp")
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(tmp), *map(str, objs)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("libmpt link failed:\n" + r.stdout.decode(errors="replace"))
    os.replace(tmp, lib_path)
    return lib_path


HOST_DIR = ROOT / "host"
HOST_TEST = HOST_DIR / "gpurenderer_parity"
HOST_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "gpurenderer_parity.cpp"]
# the display step's driver (tests/test_display_host_cpp.py): the same mirror, another main
DISPLAY_TEST = HOST_DIR / "display_views"
DISPLAY_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "display_views.cpp"]
# the denoiser's driver (tests/test_denoise_host_cpp.py)
DENOISE_TEST = HOST_DIR / "denoise_blend"
DENOISE_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "denoise_blend.cpp"]
# GPURenderer::update_vertices over several contexts (tests/test_refit_host_cpp.py)
REFIT_TEST = HOST_DIR / "refit_move"
REFIT_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "refit_move.cpp"]
# GPURenderer::rebuild_bvh over several contexts (tests/test_rebuild_host_cpp.py)
REBUILD_TEST = HOST_DIR / "rebuild_move"
REBUILD_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "rebuild_move.cpp"]
# GPURenderer::rebuild_bvh in PLOC mode (tests/test_ploc_host_cpp.py)
PLOC_TEST = HOST_DIR / "ploc_move"
PLOC_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "ploc_move.cpp"]
# GPURenderer::set_scene with a build mode (tests/test_upload_host_cpp.py)
UPLOAD_TEST = HOST_DIR / "upload_mode"
UPLOAD_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "upload_mode.cpp"]
# GPURenderer::set_objects / update_transforms over several contexts (tests/test_xform_host_cpp.py)
XFORM_TEST = HOST_DIR / "xform_move"
XFORM_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "xform_move.cpp"]
# GPURenderer::set_skin / update_skin over several contexts (tests/test_skin_host_cpp.py)
SKIN_TEST = HOST_DIR / "skin_move"
SKIN_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "skin_move.cpp"]
# GPURenderer::set_morph / update_morph / update_morph_skin over several contexts (tests/test_morph_host_cpp.py)
MORPH_TEST = HOST_DIR / "morph_move"
MORPH_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "morph_move.cpp"]
# GPURenderer::set_animation / update_animation over several contexts (tests/test_anim_host_cpp.py)
ANIM_TEST = HOST_DIR / "anim_move"
ANIM_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "anim_move.cpp"]
# GPURenderer::set_normals / get_vertices over several contexts (tests/test_normals_host_cpp.py)
NORMALS_TEST = HOST_DIR / "normals_move"
NORMALS_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "normals_move.cpp"]
# GPURenderer::set_temporal / denoise_temporal (tests/test_temporal_host_cpp.py)
TEMPORAL_TEST = HOST_DIR / "temporal_move"
TEMPORAL_SOURCES = [HOST_DIR / "gpu_renderer.cpp", ROOT.parent / "tests" / "cpp" / "temporal_move.cpp"]


def _build_driver(exe: Path, sources, lib: Path, verbose: bool) -> Path:
    deps = list(sources) + sorted(HOST_DIR.glob("*.h")) + [lib]
    if exe.exists() and all(p.stat().st_mtime <= exe.stat().st_mtime for p in deps):
        return exe
    # the drivers also call the HIP runtime API themselves (hipMalloc'd display buffers)
    cmd = ["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{INCLUDE}", f"-I{HOST_DIR}", "-I/opt/rocm/include",
           *map(str, sources), f"-L{PKG_DIR}", "-lmpt", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,$ORIGIN/../mpt", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)]
    if verbose:
        print("[mpt build]", " ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("host test build failed:\n" + r.stdout.decode(errors="replace"))
    return exe


def build_host_test(verbose: bool = True) -> Path:
    """The C++ GPURenderer mirror (host/) linked with libmpt into the test drivers of
    tests/test_host_cpp.py, tests/test_display_host_cpp.py, tests/test_denoise_host_cpp.py and
    tests/test_refit_host_cpp.py, tests/test_rebuild_host_cpp.py, tests/test_ploc_host_cpp.py,
    tests/test_upload_host_cpp.py, tests/test_xform_host_cpp.py, tests/test_skin_host_cpp.py,
    tests/test_morph_host_cpp.py, tests/test_anim_host_cpp.py, tests/test_normals_host_cpp.py, tests/test_temporal_host_cpp.py (plain g++: the host side is
    ordinary C++ over the C ABI)."""
    lib = build(verbose=verbose)
    _build_driver(DENOISE_TEST, DENOISE_SOURCES, lib, verbose)
    _build_driver(DISPLAY_TEST, DISPLAY_SOURCES, lib, verbose)
    _build_driver(REFIT_TEST, REFIT_SOURCES, lib, verbose)
    _build_driver(REBUILD_TEST, REBUILD_SOURCES, lib, verbose)
    _build_driver(PLOC_TEST, PLOC_SOURCES, lib, verbose)
    _build_driver(UPLOAD_TEST, UPLOAD_SOURCES, lib, verbose)
    _build_driver(XFORM_TEST, XFORM_SOURCES, lib, verbose)
    _build_driver(SKIN_TEST, SKIN_SOURCES, lib, verbose)
    _build_driver(MORPH_TEST, MORPH_SOURCES, lib, verbose)
    _build_driver(ANIM_TEST, ANIM_SOURCES, lib, verbose)
    _build_driver(NORMALS_TEST, NORMALS_SOURCES, lib, verbose)
    _build_driver(TEMPORAL_TEST, TEMPORAL_SOURCES, lib, verbose)
    return _build_driver(HOST_TEST, HOST_SOURCES, lib, verbose)


if __name__ == "__main__":
    args = sys.argv[1:]
    defs = [a for a in args if a.startswith("-D")]
    outs = [a[len("--out="):] for a in args if a.startswith("--out=")]
    print(build(force="--force" in args, defines=defs, out=Path(outs[0]) if outs else None))
