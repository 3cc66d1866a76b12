"""Host check of csrc/carve.hpp (tests/cpp/driver_layout_check.cpp): the workspace description of every composite
driver (shortint apply, the three radix composites, the sum / mul pass, bit extraction, circuit bootstrap) counts the
bytes of its closed form, and carved on a heap block of exactly that size its arrays are aligned, ordered, disjoint and
writable at both ends under ASan + UBSan; a mis-ordered description is aligned up.  No GPU: the header has no HIP in
it, so the host compiler builds the program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CXX), reason="no host C++ compiler")
def test_every_workspace_counts_its_closed_form_and_carves_inside_it(tmp_path):
    exe = str(tmp_path / "driver_layout_check")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tfhe-rs-main_modified_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "driver_layout_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    m = re.search(r"^driver layouts: (\d+) cases, 0 failures$", out.stdout, re.M)
    assert m and int(m.group(1)) >= 200, out.stdout[-4000:]
