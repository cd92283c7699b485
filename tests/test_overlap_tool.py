"""tools/overlap_from_trace.py on a hand-written kernel trace with known overlaps (CPU only).

tests/golden/overlap_trace_small.csv, times in ns, two render streams (queues 1 and 2):
  a counted pass (TALLY fused launch) and a warm-up pass, both before the timed region;
  pass A, queue 1: init 1000-1010, fused 1010-1400 and 1400-1600, combine 1600-1700 and 1700-1750
  pass B, queue 2: init 1005-1020, fused 1500-1900, combine 1920-2000
  a caller's kernel on queue 9 at 1905-1915, and one after the region (2100-2150).
Window 1000-2000. Fused runs 1010-1900 (890); the combines of A lie under B's fused launch
(150 of `both`), B's combine runs alone (80); 1000-1010 and 1905-1915 hold other kernels only
(20); 1900-1905 and 1915-1920 hold nothing (10). Of the combines' 230 ns, 150 are overlapped.
"""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TOOL = os.path.join(HERE, "..", "tools", "overlap_from_trace.py")
TRACE = os.path.join(HERE, "golden", "overlap_trace_small.csv")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("overlap_from_trace", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ns_per_frame(ms):
    return ms * 1e6


def test_known_overlaps(tool):
    r = tool.analyse(tool.read_trace(TRACE), steps=4, batch=2)
    assert r["passes"] == 2 and r["streams"] == 2
    want = {"window": 1000, "fused": 890, "both": 150, "combine_alone": 80, "other_only": 20, "idle": 10,
            "fused_dispatch": 990, "combine_dispatch": 230}
    for k, ns in want.items():
        assert ns_per_frame(r[k + "_ms_per_frame"]) == pytest.approx(ns / 4, abs=1e-6), k
    assert r["combine_overlapped_share"] == pytest.approx(150 / 230, abs=1e-12)
    # the four states and the other-kernel time tile the window
    parts = r["fused_ms_per_frame"] + r["combine_alone_ms_per_frame"] + r["other_only_ms_per_frame"] + r["idle_ms_per_frame"]
    assert parts == pytest.approx(r["window_ms_per_frame"], abs=1e-12)


def test_counted_and_earlier_passes_are_left_out(tool):
    rows = tool.read_trace(TRACE)
    assert len(tool.passes_of(rows)) == 4
    # three uncounted passes exist: the warm-up pass joins a region of three
    r = tool.analyse(rows, steps=6, batch=2)
    assert ns_per_frame(r["window_ms_per_frame"]) * 6 == pytest.approx(2000 - 200, abs=1e-6)
    # ... and the counted pass never does
    with pytest.raises(SystemExit):
        tool.analyse(rows, steps=8, batch=2)
    # --skip-last: the passes after the timed region
    r = tool.analyse(rows, steps=2, batch=2, skip_last=2)
    assert ns_per_frame(r["window_ms_per_frame"]) * 2 == pytest.approx(320 - 200, abs=1e-6)
    assert r["combine_overlapped_share"] == 0.0


def test_classes(tool):
    assert tool.classify("void rtamd::wf_trace_fused<false, false, 15, false>(rtamd::DevScene)") == tool.FUSED
    assert tool.classify("rtamd::wf_combine_parents_co(rtamd::DevScene)") == tool.COMBINE
    assert tool.is_counted("void rtamd::wf_trace_fused<false, false, 15, true, false>(x)")
    assert not tool.is_counted("void rtamd::wf_trace_fused<false, false, 15, false, true>(x)")
    assert not tool.is_counted("rtamd::wf_combine_parents(x)")


def test_command_line(tmp_path):
    out = subprocess.run([sys.executable, TOOL, TRACE, "--steps", "4", "--batch", "2", "--json"], check=True,
                         capture_output=True, text=True).stdout
    r = json.loads(out)
    assert r["combine_overlapped_share"] == pytest.approx(150 / 230, abs=1e-12)
    text = subprocess.run([sys.executable, TOOL, TRACE, "--steps", "4", "--batch", "2"], check=True,
                          capture_output=True, text=True).stdout
    assert "65.2 %" in text
    bad = tmp_path / "bad.csv"
    bad.write_text('"Kernel_Name","Start_Timestamp"\n"k",1\n')
    assert subprocess.run([sys.executable, TOOL, str(bad)], capture_output=True).returncode != 0
