"""Things left running: a session, the CLI under a pipe and the reference's per-buffer seams over thousands of calls -- frames keep coming out right and
the process does not grow.  Round 6 found 2 .. 3.6 KB of heap per segment here: the HIP runtime keeps its records of finished copies until somebody
synchronises their STREAM (tools/hip_retained_commands.py); hip_util.hpp (blocking_copy, kReapEvery) is what these tests hold in place.  Short forms of
tools/soak.py, tools/soak_cli.py, tools/soak_seams.py (the long ones: tools/gpu/soak.sh, profiles/r06_soak_*.json)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_a_session_fed_in_live_sized_segments_does_not_grow():
    import soak
    out = soak.run(streams=4, loop_tf=125, total_tf=2600, calls=2, oracle_tf=140)
    assert out["ok"], out
    assert out["memory"]["samples"] >= 4 and out["memory"]["flat"]
    heap = out["memory"]["heap_in_use_kb_by_sample"]
    assert heap[-1] - heap[0] < 1024, heap              # (before: 3.6 KB per feed = 5 MB over these samples)
    assert all(out["oracle"]["first_frames_equal"]) and out["frames_that_differ"][0] == 0 and out["frames_that_differ"][1] == 0


def _tool(name, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + list(args), capture_output=True, text=True, timeout=600, env=e)
    line = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert line, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.returncode, json.loads(line[-1])


def test_the_cli_under_a_pipe_does_not_grow():
    rc, out = _tool("soak_cli.py", "--total-tf", "3000")
    assert rc == 0 and out["ok"], out
    assert out["eti_frames"] == out["expected"] == 4 * (3000 - 15)
    assert out["rss_anon_growth_kb_over_the_second_half"] < 1024, out["rss_anon_kb_by_sample"]    # (before: 2 KB per segment = 2.3 MB here)


def test_the_reference_call_pattern_through_the_seams_does_not_grow():
    rc, out = _tool("soak_seams.py", "--calls", "3000", "--oracle-tf", "150")
    assert rc == 0 and out["ok"], out
    assert out["oracle"]["equal"] and out["frames_that_differ"] == 0 and out["heap_growth_kb_over_the_second_half"] < 512
