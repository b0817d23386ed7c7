"""The trainer's C ABI from plain C (tests/c/cabi_check_train.c, the sibling of cabi_check.c): the eight s2s_trainer_* symbols resolve,
s2s_adam fills from C, and every refusal that needs no GPU -- NULL out / cfg / blob, a mode other than generic-geometry, a refused
size, a wrong blob size, NULL trainers -- answers with its code and message."""
import os
import subprocess

from seq2squiggle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c_consumer_of_the_trainer(tmp_path):
    exe = tmp_path / "cabi_check_train"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "cabi_check_train.c"), "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe), _lib._LIB_DEFAULT], capture_output=True, text=True)
    assert r.returncode == 0 and "CABI_TRAIN_OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
    for name in ("s2s_trainer_create", "s2s_trainer_destroy", "s2s_trainer_last_error", "s2s_trainer_set_memory", "s2s_trainer_micro_batch",
                 "s2s_trainer_weights", "s2s_trainer_gradients", "s2s_trainer_step"):
        assert name in _lib.EXPORTS
