"""Key sets that grow through the C++ host mirror (include/dusk_schnorr.hpp: KeySet*::append): compile
tests/cpp/test_keyed_append.cpp — sign, register some keys, append the others, verify_batch by key index, bool for
bool against the per-object `PublicKey*::verify` — against libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

from cpp_build import compile_program


def test_cpp_keyed_append_compiles():
    assert os.path.exists(compile_program("test_keyed_append"))


@pytest.mark.gpu
def test_cpp_keyed_append_matches_per_object_verify_on_gpu():
    out = subprocess.run([compile_program("test_keyed_append")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
