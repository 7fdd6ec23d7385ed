"""Registered key sets through the C++ host mirror (include/dusk_schnorr.hpp: KeySet, KeySetDouble, KeySetVarGen):
compile tests/cpp/test_keyed.cpp — sign, register, verify_batch by key index, bool for bool against the
per-object `PublicKey*::verify` — against libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

from cpp_build import compile_program


def test_cpp_keyed_compiles():
    assert os.path.exists(compile_program("test_keyed"))


@pytest.mark.gpu
def test_cpp_keyed_matches_per_object_verify_on_gpu():
    out = subprocess.run([compile_program("test_keyed")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
