"""The positioned key-major database (ipkgpu_score_groups_keymajor_positions_device): declared, exported and bound.
A context cannot be created without a GPU, so nothing more runs here; tests/test_gpu_positions_db.py does the rest."""
import ctypes
import os
import re

import ipk_amd
from ipk_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ipkgpu_score_groups_keymajor_positions_device", "ipkgpu_parts_positions_device", "ipkgpu_db_positions",
       "ipkgpu_db_positions_device"]


def test_header_declares_the_positioned_call():
    text = open(os.path.join(ROOT, "include", "ipkgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/ipkgpu.h"


def test_library_exports_the_positioned_call():
    lib = ipk_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"libipkgpu.so does not export {name}"


def test_engine_binds_the_positioned_call():
    lib = ipk_amd.load_library()
    E._bind_keymajor(lib)
    assert lib.ipkgpu_score_groups_keymajor_positions_device.argtypes == lib.ipkgpu_score_groups_keymajor_device.argtypes
    assert lib.ipkgpu_db_positions.restype == ctypes.POINTER(ctypes.c_uint32)
    for name in NEW:
        assert name in E.ABI_SYMBOLS
    assert callable(E.Engine.score_groups_keymajor_positions)
    assert callable(E.Parts.positions_tensor) and callable(E.Db.positions) and callable(E.Db.positions_device_ptr)
    # without a context the accessors answer "none" instead of faulting
    assert not lib.ipkgpu_parts_positions_device(None) and not lib.ipkgpu_db_positions_device(None)
