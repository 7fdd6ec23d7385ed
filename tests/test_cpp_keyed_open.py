"""Key sets as a key cache through the C++ host mirror (include/dusk_schnorr.hpp: KeySet*::verify_batch_open*):
compile tests/cpp/test_keyed_open.cpp — sign, register some of the keys, verify_batch_open over the arguments of
verify_batch, bool for bool against the free verify_batch*, the miss count as constructed, the submit form — against
libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_keyed_open.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_keyed_open")


def _compile():
    from schnorr_amd import _lib
    _lib.load()
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC,
           "-L", os.path.join(ROOT, "schnorr_amd"), "-ldsv", "-Wl,-rpath," + os.path.join(ROOT, "schnorr_amd")]
    subprocess.check_call(cmd)


def test_cpp_keyed_open_compiles():
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_keyed_open_matches_verify_batch_on_gpu():
    _compile()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
