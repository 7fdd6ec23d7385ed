"""Key sets that grow through the C++ host mirror (include/dusk_schnorr.hpp: KeySet*::append): compile
tests/cpp/test_keyed_append.cpp — sign, register some keys, append the others, verify_batch by key index, bool for
bool against the per-object `PublicKey*::verify` — against libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_keyed_append.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_keyed_append")


def _compile():
    from schnorr_amd import _lib
    _lib.load()
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC,
           "-L", os.path.join(ROOT, "schnorr_amd"), "-ldsv", "-Wl,-rpath," + os.path.join(ROOT, "schnorr_amd")]
    subprocess.check_call(cmd)


def test_cpp_keyed_append_compiles():
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_keyed_append_matches_per_object_verify_on_gpu():
    _compile()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
