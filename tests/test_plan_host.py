"""CPU tier of the gather's work plan (``csrc/rgcn_plan.h``): ``tests/plan_check.cpp`` plans rowptr arrays - single
segments at the level thresholds, the run / pack boundaries, seeded random graphs with hubs of two and three levels -
executes every plan symbolically in integers and holds it to the plan the planner gave before it moved into the
header, stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer (their runtimes are linked INTO the program).

``RGCN_PLAN_CHECK_FULL=1`` adds the top of the int32 range, ``rowptr = {0, 2147483646}`` and ``{0, 100, 2147483646}``,
where the pack cuts do not fit an int32: about a minute and 1.1 GB under the sanitizers (measured: 55.8 s, 1110 MB peak
resident), against 1.5 s for the rest - too long for every run of the suite."""
import os

import pytest

from conftest import ROOT


def test_plans_execute_to_the_segment_sums_and_are_the_parents_plans_under_sanitizers(tmp_path):
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                    os.path.join(ROOT, "tests", "plan_check.cpp"), "-o", str(exe)], check=True)
    full = os.environ.get("RGCN_PLAN_CHECK_FULL") == "1"
    done = subprocess.run([str(exe)] + (["--full"] if full else []), capture_output=True, text=True)
    last = done.stdout.strip().splitlines()[-1] if done.stdout.strip() else ""
    assert done.returncode == 0 and last.startswith("plan_check ok 20"), done.stdout[-2000:] + done.stderr[-2000:]
    assert last.endswith("top of range") == full
    # the thresholds, as the program printed them: a third level at 131,073 edges, a fourth at 67,108,865
    table = {line.split()[0]: line.split()[1] for line in done.stdout.splitlines()[1:] if line and line[0].isdigit()}
    assert (table["131072"], table["131073"], table["67108864"], table["67108865"]) == ("2", "3", "3", "4")


def test_plan_header_has_no_device_code_and_the_library_uses_it():
    csrc = os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc")
    header = open(os.path.join(csrc, "rgcn_plan.h")).read()
    assert "hip_runtime" not in header and "__global__" not in header and "__device__" not in header
    assert '#include "rgcn_plan.h"' in open(os.path.join(csrc, "rgcn_common.h")).read()
    graph = open(os.path.join(csrc, "rgcn_graph.hip")).read()
    assert "rgcn_build_plan(" in graph and "stable_sort" not in graph          # one planner: the header's
