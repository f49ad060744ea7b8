"""CPU tier of the row stream's block deal (csrc/rowdeal.inc: block number -> rows of a frame, the one function phase 1's
drawn deal and its test share).  The source text the device code includes is built by g++ with -fsanitize=address,undefined
into a program with its own main (csrc/rowdeal_main.cc), which checks, exhaustively for frame heights 1..260, 3 and 4 rows
per block, both orders (outside in block by block and in runs of 8) and 8 and 16 waves' worth of draws, that the blocks cover every row exactly once, that none leaves
[0, bh), that the block at the frame's end is cut and not wrapped, that numbers drawn past the end are empty, and that the
row loop (two buffers, the draw two blocks ahead) reduces every row once.  A child process: nothing is loaded into this
interpreter and nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")


def test_block_deal_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "rowdeal-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "rowdeal_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "rowdeal host code ok (3120 cases)" in r.stdout, tail
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


def test_the_device_code_includes_the_same_text():
    """phase 1 calls rowdeal_block of rowdeal.inc, and the one translation unit includes that file before phase1.inc."""
    unit = open(os.path.join(CSRC, "tsdf_hip.hip")).read()
    assert unit.index('#include "rowdeal.inc"') < unit.index('#include "phase1.inc"')
    assert "rowdeal_block(" in open(os.path.join(CSRC, "phase1.inc")).read()
