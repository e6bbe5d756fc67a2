"""Every host build the tests make of the sources under tests/emul/: the device cores as shared libraries and as sanitized
stand-alone programs, and the drivers that link libopencv-ar.  One flag set, one temporary directory per process, every result
built once per process.  (conftest.py's `emul` fixture keeps its own libemul.so; helpers._build runs make.)"""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import helpers as H

CSRC = os.path.join(H.PKG, "csrc")
INCLUDE = os.path.join(H.ROOT, "include")
EMUL = os.path.join(H.ROOT, "tests", "emul")
CORE_FLAGS = ["-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
              "-I" + CSRC, "-I" + INCLUDE]
TILED = ["-DOCVAR_NBR_TILED"]


@functools.lru_cache(maxsize=None)
def _out_dir():
    d = tempfile.mkdtemp(prefix="ocvar_hostbuild_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _compile(flags, out, name, tail=()):
    path = os.path.join(_out_dir(), out)
    subprocess.check_call(["g++"] + flags + ["-o", path, os.path.join(EMUL, name + ".cpp")] + list(tail))
    return path


@functools.lru_cache(maxsize=None)
def host_core(name, tiled=True):
    """tests/emul/<name>.cpp as a shared library -> its ctypes.CDLL (argtypes and restype are the caller's).  Every caller of a
    name gets the same CDLL object, so callers that declare the same function must declare it alike."""
    flags = ["-O2"] + CORE_FLAGS + (TILED if tiled else []) + ["-shared"]
    return C.CDLL(_compile(flags, "lib%s%s.so" % (name, "" if tiled else "_untiled"), name))


@functools.lru_cache(maxsize=None)
def sanitized_program(name, main_macro):
    """tests/emul/<name>.cpp with its stand-alone main under AddressSanitizer and UndefinedBehaviorSanitizer -> the program's path"""
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D" + main_macro] + CORE_FLAGS + TILED
    return _compile(flags, name + "_san", name)


def run_sanitized(name, main_macro, expect, timeout):
    """runs the sanitized program: it ends with status 0, says `expect`, and no sanitizer reports"""
    r = subprocess.run([sanitized_program(name, main_macro)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert expect in r.stdout, r.stdout[-2000:]
    assert "runtime error" not in r.stderr, r.stderr[-2000:]


@functools.lru_cache(maxsize=None)
def host_driver(name):
    """tests/emul/<name>.cpp linked against libopencv-ar -> the program's path"""
    lib = os.path.join(H.PKG, "lib")
    return _compile(["-O2", "-std=c++17", "-I" + INCLUDE, "-I" + os.path.join(INCLUDE, "shim")], name, name,
                    ["-L" + lib, "-lopencv-ar", "-Wl,-rpath," + lib])
