"""CPU: a plain bench.py run stops at its headline; --full adds the roofline, the CPU baseline, the mask IoU vs the oracle, the
workload's extra figures and the single-GPU variants after the timed steps, and the --no-* switches leave parts of a --full run out."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


class RecordingWorkload:
    """stands in for a workload: records which of the --full items ran, in order"""

    def __init__(self):
        self.calls = []

    def roofline(self):
        self.calls.append("roofline")
        return {"bound": "mfma"}

    def cpu_baseline(self, seconds):
        self.calls.append("cpu_baseline")
        return {"value": 0.1, "seconds": seconds}

    def mask_iou_vs_oracle(self):
        self.calls.append("mask_iou_vs_oracle")
        return {"iou_min": 1.0}

    def extra(self):
        self.calls.append("extra")
        return {"warp_chain": {"us_per_frame": 60.0}}

    def variants(self):
        self.calls.append("variants")
        return {"batch1": {"frames_per_s": 70.0, "ms_per_frame": 14.3}, "batch1_lanes3": {"frames_per_s": 80.0}}


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1", *argv])
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    assert parse(monkeypatch).full is False
    assert parse(monkeypatch, "--full").full is True


def test_full_report_runs_every_item_once(monkeypatch):
    wl, out = RecordingWorkload(), {}
    bench.full_report(out, wl, parse(monkeypatch, "--full", "--cpu-seconds", "5"), 1)
    assert wl.calls == ["roofline", "cpu_baseline", "mask_iou_vs_oracle", "extra", "variants"]
    assert list(out) == ["roofline", "cpu_baseline", "mask_iou_vs_oracle", "warp_chain", "variants", "batch1"]
    assert out["cpu_baseline"]["seconds"] == 5.0
    assert out["batch1"]["frames_per_s"] == 70.0 and out["batch1"]["frames_per_s_3_in_flight"] == 80.0


def test_no_switches_leave_parts_of_a_full_run_out(monkeypatch):
    wl, out = RecordingWorkload(), {}
    bench.full_report(out, wl, parse(monkeypatch, "--full", "--no-roofline", "--no-cpu-baseline", "--no-iou", "--no-variants"), 1)
    assert wl.calls == ["extra"]
    assert out == {"roofline": None, "warp_chain": {"us_per_frame": 60.0}}


def test_multi_rank_full_report_keeps_the_single_gpu_items_out(monkeypatch):
    wl, out = RecordingWorkload(), {}
    bench.full_report(out, wl, parse(monkeypatch, "--full"), 2)
    assert wl.calls == ["roofline", "extra"]
