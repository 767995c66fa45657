"""The positioned database on several ranks (ipkgpu_score_groups_keymajor_positions_owners_device,
ipkgpu_merge_parts_positions_ptrs): declared, exported and bound.  A context cannot be created without a GPU, so nothing more runs
here; tests/test_gpu_positions_ranks.py does the rest."""
import ctypes
import os
import re

import ipk_amd
from ipk_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ipkgpu_score_groups_keymajor_positions_owners_device", "ipkgpu_merge_parts_positions_ptrs"]


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "ipkgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/ipkgpu.h"


def test_library_exports_the_calls():
    lib = ipk_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"libipkgpu.so does not export {name}"


def test_engine_binds_the_calls():
    lib = ipk_amd.load_library()
    E._bind_keymajor(lib)
    assert lib.ipkgpu_score_groups_keymajor_positions_owners_device.argtypes == lib.ipkgpu_score_groups_keymajor_device.argtypes
    assert lib.ipkgpu_score_groups_keymajor_positions_owners_device.restype == ctypes.c_int
    # the plain merge's arguments with the positions array in front of the out pointer
    plain = list(lib.ipkgpu_merge_parts_ptrs.argtypes)
    assert list(lib.ipkgpu_merge_parts_positions_ptrs.argtypes) == plain[:-1] + [ctypes.POINTER(ctypes.c_void_p), plain[-1]]
    assert lib.ipkgpu_merge_parts_positions_ptrs.restype == ctypes.c_int
    for name in NEW:
        assert name in E.ABI_SYMBOLS
    assert callable(E.Engine.score_groups_keymajor_positions_owners) and callable(E.Engine.merge_parts_positions_ptrs)
    assert callable(E.Engine.exchange_begin) and callable(E.Engine.exchange_merge)
    # without a context both calls answer "invalid" instead of faulting
    out = ctypes.c_void_p()
    assert lib.ipkgpu_score_groups_keymajor_positions_owners_device(None, None, 0, 0, 20, None, 4, ctypes.c_float(-1.0), 2, ctypes.byref(out)) == 1
    assert lib.ipkgpu_merge_parts_positions_ptrs(None, 20, 4, 0, 2, 1, None, None, None, ctypes.byref(out)) == 1
