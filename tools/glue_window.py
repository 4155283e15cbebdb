"""The per-frame depth glue of a bench step in a rocprofv3 --kernel-trace CSV of tools/step_trace.py (kernel trace only: no counters,
no other tracing in that run).  Per step of 8 frames:
  post-join window : from the end of the last net kernel (a layer-program kernel: `csmconv::` in its signature) before the step's
                     first k_tile_bin to the start of that k_tile_bin -- (a) its wall time, (b) the share of it covered by at least
                     one running kernel, (c) the launches that start inside it, (d) the host reads of the glue's stats PER STEP (a
                     kernel trace does not show host reads: this is the count `stats_reads` that `step_trace.py --count` prints
                     in a run of its own -- pass that run's output file; by the code all of them fall into this window, the
                     trace does not prove it)
  depth post       : (e) the same for the depth stream's post-processing in front of the join -- from the end of the last net kernel
                     on a depth queue before the step's first post-processing kernel to the end of its last one; launches and
                     coverage are those of the queues that run post-processing kernels (one per depth stream); host reads: this
                     code path has none (read off the code, not measured)
  det -> refine    : (f) the detector's post-processing chain on the main queue (the queue that runs k_refine_batch) -- from the end
                     of the step's last RTMDet program kernel (the last `csmconv::` kernel on that queue before the step's first
                     k_nms_mask) to the start of its first ISNet program kernel (the first `csmconv::` kernel on that queue after the
                     step's first k_refine_batch): wall time, launches on that queue and the share of the window that queue covers
                     (the depth streams keep the GPU busy meanwhile; the detector's host read falls into this window)
usage: python tools/glue_window.py <kernel_trace.csv> [step_trace output] [frames per step, default 8] [steps to report, default 6]"""
import csv
import re
import sys

DEPTH_POST = ("k_leres_quantize", "k_resize_u8_to_f32", "k_resize_u8_lanczos4", "k_minpos_scan", "k_minpos_apply", "k_lpost_")


def union_ns(iv):
    tot, cs, ce = 0, None, None
    for s, e in sorted(iv):
        if cs is None:
            cs, ce = s, e
        elif s > ce:
            tot += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    return tot + (ce - cs if cs is not None else 0)


def main():
    path = sys.argv[1]
    trace_out = sys.argv[2] if len(sys.argv) > 2 else None
    fps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    nsteps = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "0")))
    rows.sort()
    bins = [r for r in rows if "k_tile_bin" in r[2]]
    allfirsts = [bins[i] for i in range(0, len(bins), fps)]
    firsts = allfirsts[-nsteps:]
    reads = None
    if trace_out:
        m = re.search(r"stats_reads ([0-9.]+)", open(trace_out).read())
        reads = float(m.group(1)) if m else None
    print("%d k_tile_bin launches = %d steps of %d frames; the last %d steps:" % (len(bins), len(bins) // fps, fps, len(firsts)))
    print("post-join window (end of the last net kernel -> start of the step's first k_tile_bin)")
    print("  step   (a) wall us   (b) covered %   (c) launches   (d) stats reads per step (step_trace.py --count, not from the trace)")
    tot = [0.0, 0.0, 0]
    prev_end = allfirsts[-nsteps - 1][0] if len(allfirsts) > nsteps else rows[0][0]       # the step before the first reported one
    ends = []
    names = {}
    for i, fb in enumerate(firsts):
        nets = [r for r in rows if r[1] <= fb[0] and "csmconv::" in r[2]]
        t0 = max(r[1] for r in nets)
        inside = [r for r in rows if t0 <= r[0] < fb[0]]
        cov = union_ns([(max(s, t0), min(e, fb[0])) for s, e, _, _ in rows if e > t0 and s < fb[0]])
        wall = fb[0] - t0
        print("  %4d   %11.1f   %13.1f   %12d   %s" % (i, wall / 1e3, 100.0 * cov / max(wall, 1), len(inside),
                                                      "not counted" if reads is None else "%.0f" % reads))
        tot[0] += wall; tot[1] += cov; tot[2] += len(inside)
        for r in inside:
            k = re.sub(r"[<(].*", "", r[2].replace("void ", "").replace("(anonymous namespace)::", ""))[:60]
            v = names.setdefault(k, [0, 0])
            v[0] += 1; v[1] += r[1] - r[0]
        ends.append((prev_end, t0))
        prev_end = fb[0]
    n = len(firsts)
    print("  mean   %11.1f   %13.1f   %12.1f" % (tot[0] / n / 1e3, 100.0 * tot[1] / max(tot[0], 1), tot[2] / n))
    print("  launches in the window, per step (kernel time us):")
    for k, v in sorted(names.items(), key=lambda kv: -kv[1][1]):
        print("    %6.1f x  %8.1f us  %s" % (v[0] / n, v[1] / n / 1e3, k))
    print("depth post-processing in front of the join (the queues of the depth streams; the code path has no host read: not measured)")
    print("  step   (a) wall us   (b) covered %   (c) launches")
    tot = [0.0, 0.0, 0]
    for i, (lo, hi) in enumerate(ends):
        post = [r for r in rows if lo < r[0] < hi and any(k in r[2] for k in DEPTH_POST)]
        if not post:
            print("  %4d   no depth post-processing kernel found" % i)
            continue
        qs = {r[3] for r in post}                                   # one queue per depth stream
        nets = [r for r in rows if r[3] in qs and r[1] <= post[0][0] and "csmconv::" in r[2]]
        t0, t1 = max(r[1] for r in nets), max(r[1] for r in post)
        inside = [r for r in rows if r[3] in qs and t0 <= r[0] < t1]
        cov = union_ns([(s, e) for s, e, _, _ in inside])
        wall = t1 - t0
        print("  %4d   %11.1f   %13.1f   %12d" % (i, wall / 1e3, 100.0 * cov / max(wall, 1), len(inside)))
        tot[0] += wall; tot[1] += cov; tot[2] += len(inside)
    print("  mean   %11.1f   %13.1f   %12.1f" % (tot[0] / n / 1e3, 100.0 * tot[1] / max(tot[0], 1), tot[2] / n))
    print("detector post-processing on the main queue (end of the last RTMDet program kernel -> start of the first ISNet program kernel;")
    print("launches and coverage are those of that queue alone)")
    print("  step   (a) wall us   (b) covered %   (c) launches")
    tot = [0.0, 0.0, 0]
    names, found = {}, 0
    lo = allfirsts[-nsteps - 1][0] if len(allfirsts) > nsteps else rows[0][0]
    for i, fb in enumerate(firsts):
        step = [r for r in rows if lo <= r[0] < fb[0]]
        lo = fb[0]
        prep = [r for r in step if "k_refine_batch" in r[2]]
        nms = [r for r in step if "k_nms_mask" in r[2]]
        if not prep or not nms:
            print("  %4d   no k_nms_mask / k_refine_batch launch found" % i)
            continue
        q = prep[0][3]
        main = [r for r in step if r[3] == q]
        before = [r[1] for r in main if "csmconv::" in r[2] and r[1] <= nms[0][0]]
        after = [r[0] for r in main if "csmconv::" in r[2] and r[0] >= prep[0][1]]
        if not before or not after:
            print("  %4d   no net kernel around the window on queue %s" % (i, q))
            continue
        t0, t1 = max(before), min(after)
        inside = [r for r in main if t0 <= r[0] < t1]
        cov = union_ns([(s, min(e, t1)) for s, e, _, _ in inside])
        wall = t1 - t0
        print("  %4d   %11.1f   %13.1f   %12d" % (i, wall / 1e3, 100.0 * cov / max(wall, 1), len(inside)))
        tot[0] += wall; tot[1] += cov; tot[2] += len(inside); found += 1
        for r in inside:
            k = re.sub(r"[<(].*", "", r[2].replace("void ", "").replace("(anonymous namespace)::", ""))[:60]
            v = names.setdefault(k, [0, 0])
            v[0] += 1; v[1] += r[1] - r[0]
    if found:
        print("  mean   %11.1f   %13.1f   %12.1f" % (tot[0] / found / 1e3, 100.0 * tot[1] / max(tot[0], 1), tot[2] / found))
        print("  launches in the window, per step (kernel time us):")
        for k, v in sorted(names.items(), key=lambda kv: -kv[1][1]):
            print("    %6.1f x  %8.1f us  %s" % (v[0] / found, v[1] / found / 1e3, k))


if __name__ == "__main__":
    main()
