"""The random filter on the device (ipkgpu_db_filter_random): declared, exported and bound, and the one filter-and-write helper exists.
A context cannot be created without a GPU, so nothing more runs here; tests/test_gpu_filter_random.py does the rest."""
import ctypes
import os
import re

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ipkgpu_db_filter_random"


def test_header_declares_the_random_filter():
    text = open(os.path.join(ROOT, "include", "ipkgpu.h")).read()
    assert re.search(r"\b" + NAME + r"\s*\(", text), f"{NAME} is not declared in include/ipkgpu.h"


def test_library_exports_the_random_filter():
    assert hasattr(ipk_amd.load_library(), NAME), f"libipkgpu.so does not export {NAME}"


def test_engine_binds_the_random_filter():
    lib = ipk_amd.load_library()
    E._bind_keymajor(lib)
    assert NAME in E.ABI_SYMBOLS
    assert lib.ipkgpu_db_filter_random.restype == ctypes.c_int
    assert lib.ipkgpu_db_filter_random.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    assert callable(E.Db.filter_random)
    # without a context the call answers IPKGPU_ERR_INVALID instead of faulting
    assert lib.ipkgpu_db_filter_random(None, None) == 1


def test_one_filter_and_write_helper():
    assert callable(dbfile.filter_and_write_device)
