"""Host-only test of the act_sync spin core (ops/csrc/act_sync.h): a
stand-alone C++ program with a fake launch, built with AddressSanitizer
and UBSan and run on the CPU.  One variant sets the completion flag from
a thread, one never sets it and must time out inside its bound.

Run line (what this test does):
  c++ -std=c++17 -O1 -g -fsanitize=address,undefined
      -fno-sanitize-recover=all -pthread
      -I torch_actor_critic_amd/ops/csrc tests/native/act_sync_host.cpp
      -o act_sync_host && ./act_sync_host set && ./act_sync_host never
"""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "act_sync_host.cpp")
INC = os.path.join(REPO, "torch_actor_critic_amd", "ops", "csrc")


def _compiler():
    for c in ("c++", "g++", "clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("act_sync") / "act_sync_host")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-pthread", "-I", INC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("variant", ["set", "never"])
def test_spin_core(prog, variant):
    r = subprocess.run([prog, variant], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK " + variant), r.stdout + r.stderr
