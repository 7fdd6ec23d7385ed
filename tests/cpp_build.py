"""Compile one program of tests/cpp/ against include/ and libdsv.so: what every tests/test_cpp_*.py builds with."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(name):
    """tests/cpp/<name>.cpp -> tests/cpp/<name>, warnings on; returns the executable's path"""
    from schnorr_amd import _lib
    _lib.load()
    lib_dir = os.path.join(ROOT, "schnorr_amd")
    exe = os.path.join(ROOT, "tests", "cpp", name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, exe + ".cpp", "-L", lib_dir, "-ldsv", "-Wl,-rpath," + lib_dir])
    return exe
