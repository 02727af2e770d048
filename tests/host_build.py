"""The one builder of the CPU libraries of tests/hostemu that the test modules compile themselves: the device source of a
solver under -DSMRT_HOST_EMU, behind a small driver (tests/hostemu/*_host.cpp).

A library is stale when ANY header it could include is newer, not a hand-kept list of them: an edited kernel whose header such
a list misses is tested through an old build."""
import ctypes
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "hostemu")


def host_library(so_name, source):
    """ctypes.CDLL of tests/hostemu/<so_name>, rebuilt from tests/hostemu/<source> when stale."""
    lib, source = os.path.join(EMU_DIR, so_name), os.path.join(EMU_DIR, source)
    inputs = [source, os.path.join(ROOT, "include", "smrt_dort.h")]
    inputs += glob.glob(os.path.join(ROOT, "smrt_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(EMU_DIR, "*.hpp"))
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in inputs):
        tmp = f"{lib[:-3]}.{os.getpid()}.tmp.so"   # (several test modules, and several processes, build the same library)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DSMRT_HOST_EMU", "-I", EMU_DIR, "-o", tmp, source],
                              cwd=ROOT)
        os.replace(tmp, lib)
    return ctypes.CDLL(lib)
