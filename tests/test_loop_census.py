"""tools/loop_census.py on this tree: the tool must find the lanes = reads kernel in the compiler's output and report its loops.
Nothing here depends on how many instructions a loop has: the census is a measuring tool, profiles/trace_step_census.txt is where its
figures are kept.  (One compile of the device code, without a GPU: the slow part of this test is the compiler.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_finds_the_lanes_kernel_and_its_loops():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_census.py"), "--kernel", "ga_lanes_kernel<10, 64>"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines and lines[0].startswith("kernel ga_lanes_kernel<10, 64>"), lines[:2]
    rows = [l.split() for l in lines if l.strip().startswith(".L")]
    assert rows, "no loop found in the kernel"
    assert any("innermost" in r for r in rows)
    total = [l for l in lines if l.startswith("whole kernel")]
    assert len(total) == 1 and int(total[0].split()[2]) > 0
