"""CPU-only: the host side of the batch engine (csrc/ljmd_batch*.cpp) against its recorded transcript.  tests/batch_trace
links the batch host files with the fake HIP runtime and launchers that print their arguments, walks the ljmd_batch_* C
ABI -- every guard in the order the code checks it, the launch sequence of both precision modes with and without the g(r)
and MSD / VACF accumulators, injected launch failures and the recovery -- and prints every return code and message.
The output must equal tests/batch_trace/expected.txt byte for byte, under AddressSanitizer and UBSan: a change of the
host code that moves a launch, reorders a guard or rewords a message shows here, without a GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HERE = ROOT / "tests" / "batch_trace"


def test_batch_host_transcript():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the transcript program cannot be built")
    subprocess.run(["make", "-C", str(HERE)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(HERE / "batch_trace")], env=env, capture_output=True, timeout=120)
    stderr = out.stderr.decode(errors="replace")
    assert out.returncode == 0, (out.stdout[-2000:], stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in stderr and "runtime error:" not in stderr, stderr[-6000:]
    expected = (HERE / "expected.txt").read_bytes()
    if out.stdout != expected:
        got, want = out.stdout.split(b"\n"), expected.split(b"\n")
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail("transcript differs from expected.txt at line %d:\n  got:      %r\n  expected: %r"
                    % (k + 1, got[k] if k < len(got) else None, want[k] if k < len(want) else None))
