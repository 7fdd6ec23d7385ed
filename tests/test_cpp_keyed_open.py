"""Key sets as a key cache through the C++ host mirror (include/dusk_schnorr.hpp: KeySet*::verify_batch_open*):
compile tests/cpp/test_keyed_open.cpp — sign, register some of the keys, verify_batch_open over the arguments of
verify_batch, bool for bool against the free verify_batch*, the miss count as constructed, the submit form — against
libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

from cpp_build import compile_program


def test_cpp_keyed_open_compiles():
    assert os.path.exists(compile_program("test_keyed_open"))


@pytest.mark.gpu
def test_cpp_keyed_open_matches_verify_batch_on_gpu():
    out = subprocess.run([compile_program("test_keyed_open")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
