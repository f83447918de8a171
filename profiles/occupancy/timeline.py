"""Per-class timeline and occupancy of k_small's dispatches (profiles/occupancy/README.md).

  python profiles/occupancy/timeline.py trace <kernel_trace.csv> [sets]
      rocprofv3 --kernel-trace of bench.py: the last `sets` launch sets of k_small (a set: the
      dispatches between two gaps in which none runs), the mean over the sets of every dispatch's
      start and end relative to its set's start, per hardware queue, and each queue's idle tail.
  python profiles/occupancy/timeline.py pmc <counter_collection.csv>
      rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES (a run of its own: the profiler runs
      the dispatches one at a time), per class: a wavefront's mean life and the mean number of
      wavefronts in flight per SIMD = wave-cycles / (busy cycles x SIMDs).
"""
import collections
import csv
import sys

SIMDS, SES = 1024, 32  # MI355X: 256 CUs x 4 SIMDs; SQ_BUSY_CYCLES adds up the 32 shader engines'


def trace(path, nsets):
    rows = []
    with open(path, newline="") as f:
        for x in csv.DictReader(f):
            if "k_small<" in x["Kernel_Name"]:
                rows.append((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), int(x["Queue_Id"]),
                             int(x["Grid_Size_X"]) // 64, int(x["Workgroup_Size_X"]) // 64))
    rows.sort()
    sets, cur, end = [], [], 0
    for r in rows:
        if cur and r[0] > end:
            sets.append(cur)
            cur = []
        cur.append(r)
        end = max(end, r[1]) if len(cur) > 1 else r[1]
    sets.append(cur)
    sets = [s for s in sets if len(s) == len(sets[-1])][-nsets:]
    n = len(sets)
    span = sum(max(r[1] for r in s) - s[0][0] for s in sets) / n / 1e3
    summed = sum(r[1] - r[0] for s in sets for r in s) / n / 1e3
    print("%d sets of %d dispatches: span %.1f us, summed dispatch time %.1f us, mean overlap %.2f" % (
        n, len(sets[0]), span, summed, summed / span))
    print("| queue | families (waves) | waves/workgroup | start us | end us | duration us |")
    print("|---|---:|---:|---:|---:|---:|")
    # the same dispatch in every set: its queue, size and width (equal slices: in start order)
    keyed = []
    for s in sets:
        seen, k = collections.Counter(), {}
        for r in s:
            seen[r[2:]] += 1
            k[r[2:] + (seen[r[2:]],)] = r
        keyed.append(k)
    assert all(set(k) == set(keyed[0]) for k in keyed), "the sets differ in their dispatches"
    qend = collections.defaultdict(float)
    mean = {key: (sum(k[key][0] - s[0][0] for k, s in zip(keyed, sets)) / n / 1e3,
                  sum(k[key][1] - s[0][0] for k, s in zip(keyed, sets)) / n / 1e3) for key in keyed[0]}
    for key, (st, en) in sorted(mean.items(), key=lambda kv: (kv[0][0], kv[1][0])):
        q, fam, nw = key[:3]
        qend[q] = max(qend[q], en)
        print("| %d | %d | %d | %.1f | %.1f | %.1f |" % (q, fam, nw, st, en, en - st))
    for q in sorted(qend):
        print("queue %d idle for the last %.1f us of the span" % (q, span - qend[q]))


def pmc(path):
    d = collections.defaultdict(lambda: collections.defaultdict(list))
    with open(path, newline="") as f:
        for x in csv.DictReader(f):
            if "k_small<" not in x["Kernel_Name"]:
                continue
            k = (int(x["Grid_Size"]) // 64, int(x["Workgroup_Size"]) // 64)
            d[k][x["Counter_Name"]].append(float(x["Counter_Value"]))
            d[k]["ns"].append(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]))
    print("| families (waves) | waves/workgroup | dispatch us | wave life, cycles | waves in flight per SIMD |")
    print("|---:|---:|---:|---:|---:|")
    tw = tb = 0.0
    for (fam, nw), c in sorted(d.items(), reverse=True):
        m = {k: sum(v) / len(v) for k, v in c.items()}
        wc, busy = 4 * m["SQ_WAVE_CYCLES"], m["SQ_BUSY_CYCLES"] / SES  # (wave cycles count in quads)
        tw += wc
        tb += busy
        print("| %d | %d | %.1f | %.0f | %.2f |" % (fam, nw, m["ns"] / 1e3, wc / m["SQ_WAVES"], wc / (busy * SIMDS)))
    print("all classes: %.2f waves in flight per SIMD" % (tw / (tb * SIMDS)))


if __name__ == "__main__":
    if sys.argv[1] == "trace":
        trace(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        pmc(sys.argv[2])
