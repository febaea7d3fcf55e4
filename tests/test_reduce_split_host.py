"""CPU-only: the launch, event and stream-wait sequence of one engine step with the pair kernel in two launches
(LJMD_REDUCE_SPLIT) and without.  tests/reduce_split_host links the engine's host files with the fake HIP runtime and
recording launchers, builds an engine as ljmd_create does, runs one step as the step loop does and checks, under
AddressSanitizer and UBSan: the second launch never precedes the event recorded behind the geometry pre-pass, the second
phase of the slab reduction never precedes the join, the pair interval of the profile events ends behind the join, the
side stream has the lowest priority and is destroyed with the handle, and with the path off the sequence is the one of
the commit before it."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HERE = ROOT / "tests" / "reduce_split_host"


def test_step_sequence_with_and_without_the_split():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    subprocess.run(["make", "-C", str(HERE)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(HERE / "reduce_split_host")], env=env, capture_output=True, timeout=120)
    stdout, stderr = out.stdout.decode(errors="replace"), out.stderr.decode(errors="replace")
    assert out.returncode == 0, (stdout[-4000:], stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in stderr and "runtime error:" not in stderr, stderr[-6000:]
    assert stdout.rstrip().endswith("all ok") and "FAILED" not in stdout and "MISMATCH" not in stdout, stdout[-4000:]
