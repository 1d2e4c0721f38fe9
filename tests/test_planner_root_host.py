"""The trapezoidal ("root") tapes of the quadratic-form launch under sanitizers, on the CPU (no GPU, no HIP).

vmx_plan::plan_quad_tape plans the Q' launch over a lower-trapezoidal root L [n_masked][nq] of Q' as well (TapeProblem::k_off =
nq - n_masked): row tile mt reads k < k_off + (one past its last row), and every entry carries the index of its K segment
within its range - the slab its partial tile goes to.  tests/helpers/planner_root_driver.cpp is built with
g++ -fsanitize=address,undefined and asserts, for the small awkward shapes of tests/test_quad_root_gpu.py and the bench's
(1590 x 2512 and 3180 x 5000, four walker tiles, 512 blocks), B in {9, 64, 65, 129, 256} and four block counts: the tape's own
invariants (check_quad_tape, extended to the segments), every K range covered once, segment indices dense per range and within
the slab count the partial buffer is sized with, and k_off = 0 with rows = nq the triangle's tape entry for entry."""
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('planner_root') / 'planner_root_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'planner_root_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def test_root_tapes_under_address_and_ub_sanitizers(driver):
    run = subprocess.run([str(driver)], capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert 'FAIL' not in run.stdout and 'runtime error' not in run.stderr and 'AddressSanitizer' not in run.stderr
    assert 'all root planner checks passed' in run.stdout
    assert run.stdout.count('ok root tape') == 7 * 5 * 4          # shapes x batch sizes x block counts


def test_the_library_plans_its_root_tapes_with_the_tested_planner():
    hip = (REPO / 'vega_amd' / 'csrc' / 'vegamx.hip').read_text()
    assert 'QUAD_K_BANDS, true);' in hip and 'it->dev.nq - it->dev.n_masked}' in hip
