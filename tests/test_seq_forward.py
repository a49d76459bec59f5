"""CPU tier: the forwarding of ``rgcn_sequence_run`` (``csrc/rgcn_sequence.h``) driven stand-alone over stub entry
points, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_sequence_forwarding_over_stubs_is_exact_and_clean_under_sanitizers(tmp_path):
    """``tests/seq_forward_check.cpp`` builds a table of stubs with the library's own entry macro and runs the
    library's own loop over it: every value at its position and unchanged, wrong counts and out-of-range
    descriptors refused before any call, unknown functions unsupported, a failing call ends the run.  The
    sanitizers' runtimes are linked INTO the program, so it runs as it is, whatever the loader's environment."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "seq_forward_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                    os.path.join(ROOT, "tests", "seq_forward_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "seq_forward_check ok", done.stdout + done.stderr
