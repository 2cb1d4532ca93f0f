"""The pipelined 8K encode's timeline out of a rocprofv3 --kernel-trace CSV (tools/pipeline_timeline.sh makes one):
    python tools/pipeline_timeline.py <kernel_trace.csv> [label]
Frames are cut at the starts of the fused level-0 launches; the first three and the last frame are left out.  Per frame, relative
to its level 0: start and end of every kernel (one frame listed, the means over all); the DWT chain's busy time on the main stream;
the time in which no K3 launch (top or rest; the fallback launches do not count) is running, and in which exactly one is; the gap
between the end of top(n) and the start of top(n + 1), and between top(n)'s end and the start of the launch queued behind it."""
import csv, sys, collections


def family(k):
    if "idwt" in k:
        return None
    if "dwt53_tail" in k:
        return "tail"
    if "ht_encode_fallback" in k:
        return "fallback"
    if "ht_encode_kernel" in k:
        return "k3"
    if "pair::dwt53_pk_kernel<3" in k:          # levels 0 and 1 in one launch: it cuts the frames as level 0 does
        return "pair0+1"
    if "dwt53_pk_kernel<3" in k or "dwt_level_kernel<false, 3" in k:
        return "level0"
    if "dwt53_pk" in k or "dwt_level" in k:
        return "level"
    return None


def grid(r):
    g = 1
    for ax in "XYZ":
        g *= int(r.get("Grid_Size_" + ax, r.get("Grid_Size", 1)) or 1)
    return g


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    rows = []
    for r in csv.DictReader(open(path)):
        f = family(r["Kernel_Name"])
        if f:
            rows.append([int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3, f, grid(r)])
    rows.sort()
    k3_grids = sorted({g for _, _, f, g in rows if f == "k3"})
    for r in rows:                       # the top class has 3/4 of the blocks: the larger grid
        if r[2] == "k3":
            r[2] = "top" if r[3] == k3_grids[-1] and len(k3_grids) > 1 else "rest"
        if r[2] == "fallback":
            r[2] = "fb_top" if r[3] == max(g for _, _, f, g in rows if f == "fallback") and len({g for _, _, f, g in rows if f == "fallback"}) > 1 else "fb"
    starts = [s for s, _, f, _ in rows if f in ("level0", "pair0+1")]
    print("== %s: %d kernels, %d frames" % (label, len(rows), len(starts)))
    if len(starts) < 6:
        print("too few frames")
        return
    frames = []
    for i in range(3, len(starts) - 1):
        t0, t1 = starts[i], starts[i + 1]
        # a frame's kernels: its DWT chain starts inside [t0, t1); its K3 launches are the first of each kind that start at or after t0
        chain = [(s - t0, e - t0, f) for s, e, f, _ in rows if f in ("level0", "pair0+1", "level", "tail") and t0 <= s < t1]
        k3 = []
        for kind in ("top", "rest"):
            cand = [(s - t0, e - t0, f) for s, e, f, _ in rows if f == kind and s >= t0]
            if cand:
                k3.append(cand[0])
        frames.append(dict(period=t1 - t0, chain=chain, k3=k3, t0=t0, t1=t1))
    n = len(frames)
    mean = lambda v: sum(v) / max(len(v), 1)
    print("period (level 0 to level 0): mean %.1f us, min %.1f, max %.1f over %d frames" % (mean([f["period"] for f in frames]), min(f["period"] for f in frames), max(f["period"] for f in frames), n))
    ex = frames[n // 2]
    print("one frame (us from its level 0):")
    lv = 1 if any(f == "pair0+1" for _, _, f in ex["chain"]) else 0
    for s, e, f in ex["chain"] + ex["k3"]:
        name = f
        if f == "level":
            lv += 1
            name = "level %d" % lv
        print("    %-8s start %8.1f  end %8.1f  (%.1f)" % (name, s, e, e - s))
    # means per position of the chain
    nchain = min(len(f["chain"]) for f in frames)
    print("means over the frames:")
    for j in range(nchain):
        print("    chain[%d] %-7s start %8.1f  end %8.1f  (%.1f)" % (j, ex["chain"][j][2], mean([f["chain"][j][0] for f in frames]), mean([f["chain"][j][1] for f in frames]),
                                                                 mean([f["chain"][j][1] - f["chain"][j][0] for f in frames])))
    for j, kind in enumerate(("top", "rest")):
        v = [f["k3"][j] for f in frames if len(f["k3"]) > j]
        if v:
            print("    %-16s start %8.1f  end %8.1f  (%.1f)" % (kind, mean([x[0] for x in v]), mean([x[1] for x in v]), mean([x[1] - x[0] for x in v])))
    print("main stream busy (the DWT chain's kernels): mean %.1f us of the period; chain start to end %.1f us" % (
        mean([sum(e - s for s, e, _ in f["chain"]) for f in frames]), mean([f["chain"][-1][1] - f["chain"][0][0] for f in frames])))
    # K3 wave supply over the steady frames: launches running at each moment
    lo, hi = frames[0]["t0"], frames[-1]["t1"]
    ev = []
    for s, e, f, _ in rows:
        if f in ("top", "rest") and e > lo and s < hi:
            ev.append((max(s, lo), 1)); ev.append((min(e, hi), -1))
    ev.sort()
    depth, last, acc = 0, lo, collections.Counter()
    holes = []
    for t, d in ev:
        acc[depth] += t - last
        if depth == 0 and t - last > 0.5:
            holes.append(t - last)
        depth += d; last = t
    acc[depth] += hi - last
    print("K3 launches running (top / rest, fallback launches not counted), per frame: none %.1f us, one %.1f us, two or more %.1f us" % (
        acc[0] / n, acc[1] / n, sum(v for k, v in acc.items() if k >= 2) / n))
    print("    intervals with none: %d in %d frames, mean %.1f us, longest %.1f us" % (len(holes), n, mean(holes), max(holes or [0])))
    tops = [(s, e) for s, e, f, _ in rows if f == "top" and e > lo and s < hi]
    gaps = [tops[i + 1][0] - tops[i][1] for i in range(len(tops) - 1)]
    print("end of top(n) to start of top(n + 1): mean %.1f us, min %.1f, max %.1f (negative: they overlap)" % (mean(gaps), min(gaps or [0]), max(gaps or [0])))
    fbs = [(s, e) for s, e, f, _ in rows if f.startswith("fb") and e > lo and s < hi]
    print("fallback launches: %d, mean duration %.1f us" % (len(fbs), mean([e - s for s, e in fbs])))


if __name__ == "__main__":
    main()
