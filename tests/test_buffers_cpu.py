"""CPU: the contract of the engine's buffer owners (goldrush_amd/csrc/grp_buffers.h) where no GPU test reaches it — the
failing allocation.  tests/buffers_contract_main.cpp is built with the address and undefined-behaviour sanitizers and run
as a child process on a machine without a GPU, where every HIP allocation fails: a failed reset / ensure leaves the
owner empty, nothing is freed twice, moves leave the source empty, ensure within the capacity calls nothing."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is for machines without a GPU: it must never open one")
def test_buffer_owners_contract(tmp_path):
    exe = str(tmp_path / "buffers_contract")
    cmd = ["g++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "goldrush_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "buffers_contract_main.cpp"),
           "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    cc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "contract holds" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
