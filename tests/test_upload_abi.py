"""mpt_upload_scene_mode without a GPU: the symbol, the refusals that need no device, and the
Python wrapper's own check (tests/test_upload_gpu.py has the rest)."""
import ctypes as C
import os
import re

import pytest

import mpt
from mpt import abi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_upload_scene_mode():
    assert "mpt_upload_scene_mode" in mpt.SYMBOLS
    assert hasattr(mpt.lib(), "mpt_upload_scene_mode")
    header = open(os.path.join(ROOT, "include", "mpt.h")).read()
    assert re.search(r"^int mpt_upload_scene_mode\(MptContext\* ctx, const MptScene\* scene, int32_t mode, "
                     r"MptRebuildInfo\* info_or_NULL\);", header, re.M)


@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH, 2])
def test_null_arguments_rejected_without_a_device(cornell, mode):
    L = mpt.lib()
    s = cornell.to_abi()
    not_null = C.create_string_buffer(8)   # (never read: the NULL check comes first)
    info = abi.RebuildInfo()
    info.nodes = 77
    for ctx, sc in ((None, C.byref(s)), (None, None), (C.cast(not_null, C.c_void_p), None)):
        assert L.mpt_upload_scene_mode(ctx, sc, mode, C.byref(info)) == abi.ERR_INVALID_ARGUMENT
        assert L.mpt_last_error() == b"NULL argument"
    assert info.nodes == 77 and info.rebuilt == 0


@pytest.mark.parametrize("bad", ["sah", 1.0, True, (3,), b"\x03"])
def test_wrapper_rejects_a_non_mode_before_any_call(monkeypatch, cornell, bad):
    r = object.__new__(mpt.GPURenderer)   # no device: no context behind it
    r.h = None

    def no_call():
        raise AssertionError("the library was called")

    monkeypatch.setattr(mpt, "lib", no_call)
    monkeypatch.setattr(scene.SceneData, "to_abi", lambda self: no_call())
    with pytest.raises(TypeError, match="build must be"):
        r.set_scene(cornell, build=bad)
