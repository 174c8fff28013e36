"""Turns the rocprofv3 outputs of a profiled bench.py run (gpurun_out/<tag>/...) into the small,
committed summaries under profiles/.  Usage: python tests/prof_summarize.py gpurun_out/r01 profiles/r01
PMC units: FETCH_SIZE / WRITE_SIZE count KiB; on gfx950 FETCH_SIZE tallies 128-B requests at 64 B
(MI355X_MICROARCH.md "HBM"), so HBM read bytes = 2 * FETCH_SIZE * 1024 for wide coalesced reads."""
import collections
import csv
import glob
import json
import os
import shutil
import sys

src, dst = sys.argv[1], sys.argv[2]
os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stamp():
    """What the numbers belong to: the library build that was profiled (bench.py only uses a summary whose sha256
    equals the library it runs with) and the commit it was built from."""
    import hashlib
    import subprocess

    so = os.path.join(ROOT, "hifir_amd", "libhifir_amd.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest() if os.path.exists(so) else None
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        dirty = bool(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "hifir_amd/csrc", "include"], text=True).strip())
    except Exception:
        head, dirty = None, None
    # what the profiled run itself recorded (tests/run_profiles.sh) wins over the tree's state at summarizing time
    ran = os.path.join(src, "lib.sha256")
    if os.path.exists(ran):
        ran_sha = open(ran).read().strip()
        if ran_sha != sha:
            dirty = None  # (the tree moved on: its state says nothing about the build that ran)
        sha = ran_sha
        gh = os.path.join(src, "git_head")
        if os.path.exists(gh) and open(gh).read().strip():
            head = open(gh).read().strip()
    return {"lib_sha256": sha, "git_head": head, "csrc_dirty": dirty}



def one(pattern):
    g = glob.glob(os.path.join(src, pattern))
    return g[0] if g else None


ks = one("stats/*/*kernel_stats.csv")
if ks:
    shutil.copy(ks, dst + "_kernel_stats.csv")
bj = os.path.join(src, "bench_stats.json")
if os.path.exists(bj):
    shutil.copy(bj, dst + "_bench_under_rocprof.json")


def periodic_windows(sig, L_):
    """[(first, last)] of the whole applies in a dispatch sequence: the longest stretch in which the sequence of
    (kernel, grid) is periodic with the apply's launch count, cut into windows that end with the stretch."""
    best, cur_start = (0, 0), None
    for i in range(len(sig) - L_):
        if sig[i] == sig[i + L_]:
            if cur_start is None:
                cur_start = i
            if i + 1 - cur_start > best[1] - best[0]:
                best = (cur_start, i + 1)
        else:
            cur_start = None
    p0, p1 = best[0], best[1] + L_
    out, e = [], p1
    while e - L_ >= p0:
        out.append((e - L_, e - 1))
        e -= L_
    out.reverse()
    return out


def pmc(path, counter, bench_json):
    """per-apply counter sums of the primary workload's applies only (the hierarchy's set-up also launches kernels:
    the tail operator is formed by applying the lower levels to the identity)"""
    rows = [r for r in csv.DictReader(open(path)) if "hifamd" in r["Kernel_Name"] and r["Counter_Name"] == counter]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    L_ = int(json.loads(open(bench_json).read().strip().splitlines()[-1])["config"]["launches_per_apply"])
    wins = periodic_windows([(r["Kernel_Name"], r["Grid_Size"]) for r in rows], L_)
    napply = max(1, len(wins))
    by = collections.OrderedDict()
    for (a_, b_) in wins:
        for r in rows[a_:b_ + 1]:
            k = r["Kernel_Name"].split("(")[0].replace("void hifamd::", "").replace("hifamd::", "")
            by[k] = by.get(k, 0.0) + float(r["Counter_Value"])
    return napply, {k: v / napply for k, v in by.items()}


# agreement check the bench contract asks for: kernel time of one apply from the rocprof trace of
# the same command vs the HIP-event time bench.py reports in its JSON line
kt = one("stats/*/*kernel_trace.csv")
if kt and os.path.exists(bj):
    rows = sorted((r for r in csv.DictReader(open(kt)) if "hifamd" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    # one apply = from the level-0 S1 gather (a k_gather_scale NOT preceded by the S3 k_spmm_epi of the
    # level above) to the level-0 S7 scatter (a k_scatter_scale NOT followed by an S5 k_spmm_epi).
    # Graph replays run the nodes back to back, so the span is the sum of the node durations.  The
    # primary workload's applies come first in the run (bench.py order).
    # (S1 is fused into the first L kernel since round 2: an apply starts with whatever follows the previous apply's
    #  level-0 scatter, and ends with a k_scatter_scale that is NOT followed by an S5 product.)
    # (round 2, final: S1, S5 at level 0 and S7 are fused into the component bands, so no single kernel marks the end of
    #  an apply any more.  bench.py reports the number of graph nodes of one apply; the primary workload's timed steps
    #  replay the same node sequence back to back, so the applies are the maximal stretch in which the trace is
    #  periodic with that period, cut into windows of that many kernels.)
    line0 = json.loads(open(bj).read().strip().splitlines()[-1])
    L_ = int(line0["config"]["launches_per_apply"])
    bounds = periodic_windows([(r["Kernel_Name"], r["Grid_Size_X"]) for r in rows], L_)
    spans = [(int(rows[b_]["End_Timestamp"]) - int(rows[a_]["Start_Timestamp"])) / 1e6 for (a_, b_) in bounds]
    cnts = [L_] * len(bounds)
    first = [s_ for s_, c_ in zip(spans, cnts) if c_ == cnts[0]]
    cnt = cnts
    line = json.loads(open(bj).read().strip().splitlines()[-1])
    agree = {"applies_in_trace_primary": len(first), "kernels_per_apply": cnt[0],
             "sum_of_kernel_durations_per_apply_ms_median": sorted(first)[len(first) // 2],
             "bench_apply_ms_hip_events": line["roofline"]["apply_ms_hip_events"],
             "bench_ms_per_step_wall": line["ms_per_step"]}
    agree.update(stamp())
    json.dump(agree, open(dst + "_apply_time_agreement.json", "w"), indent=1)
    print(json.dumps(agree))
    # Per-LEVEL rooflines of the primary workload: every launch of an apply is attributed to its level and stage with
    # the library's own launch map (hifamd_launch_map, carried in the bench line) and set against the SURVEY 8(d) bytes
    # of exactly those stages (bench.py "algorithmic_bytes_by_level").  S1 runs inside the first LDU solve of a level
    # and S7 / S5 inside (or right behind) the second one, so stages are grouped by the kernels that really move their
    # bytes: in = S1 + first LDU, E = the S3 product, F+out = S5 + second LDU + S7; the tail operator (one product for
    # every level from `tail` on, dense block included) carries ALL bytes of those levels.  No group can exceed the
    # roofline by construction (bytes and time come from the same launches); a fraction > 1 is refused below.
    lmap = line["roofline"].get("launch_map")
    lbytes = line["roofline"].get("algorithmic_bytes_by_level")
    if lmap and lbytes and len(lmap) == L_:
        nlev = len(lbytes)
        grp_of = {1: "in+LDU", 2: "in+LDU", 3: "E", 4: "dense/tail", 5: "F+LDU+out", 6: "F+LDU+out", 7: "F+LDU+out"}
        to_ = line["config"].get("tail_operator") or {}
        tail_level = int(to_["level"]) if to_.get("rows") and to_.get("level", -1) >= 0 else nlev
        tms, cnt_l, per_kernel = {}, {}, {}
        napp = 0
        for (a_, b_) in bounds:
            napp += 1
            for j, q in enumerate(rows[a_:b_ + 1]):
                d_ = (int(q["End_Timestamp"]) - int(q["Start_Timestamp"])) / 1e6
                lv, stg = lmap[j] // 16, lmap[j] % 16
                key = (lv, grp_of.get(stg, "other"))
                tms[key] = tms.get(key, 0.0) + d_
                cnt_l[key] = cnt_l.get(key, 0) + 1
                kn = q["Kernel_Name"].split("(")[0].replace("void hifamd::", "").replace("hifamd::", "").split("<")[0]
                e = per_kernel.setdefault(kn, [0, 0.0])
                e[0] += 1
                e[1] += d_
        table, tot_ms, tot_b = [], 0.0, 0.0
        for lv in range(nlev):
            lb = {int(k): v for k, v in lbytes[str(lv)].items()}
            if lv > tail_level:
                continue  # (inside the tail operator)
            if lv == tail_level:
                bts = {"dense/tail": sum(sum(float(v) for v in lbytes[str(q)].values()) for q in range(lv, nlev))}
            else:
                bts = {"in+LDU": lb[1] + lb[2], "E": lb[3], "dense/tail": lb[4], "F+LDU+out": lb[5] + lb[6] + lb[7]}
            row = {"level": lv, "groups": {}}
            lms, lby = 0.0, 0.0
            for g_, by_ in bts.items():
                ms_ = tms.get((lv, g_), 0.0) / napp
                if by_ == 0 and ms_ == 0:
                    continue
                gbs = by_ / (ms_ * 1e-3) / 1e9 if ms_ > 0 else None
                if gbs is not None and gbs / 8000.0 > 1.0:
                    raise SystemExit(f"level {lv} group {g_}: {gbs:.0f} GB/s exceeds the roofline -- bytes and launches do not match")
                row["groups"][g_] = {"launches": cnt_l.get((lv, g_), 0) / napp, "ms": ms_, "algorithmic_bytes": by_, "GBs": gbs,
                                     "frac_of_8TBs": gbs / 8000.0 if gbs else None}
                lms += ms_
                lby += by_
            row.update({"ms": lms, "algorithmic_bytes": lby, "GBs": lby / (lms * 1e-3) / 1e9 if lms else None,
                        "frac_of_8TBs": lby / (lms * 1e-3) / 8e12 if lms else None})
            if lv == tail_level:
                row["note"] = f"levels {lv}..{nlev - 1} and the dense block as ONE operator product"
            table.append(row)
            tot_ms += lms
            tot_b += lby
        stages = {"per_level": table, "total": {"ms": tot_ms, "algorithmic_bytes": tot_b, "GBs": tot_b / (tot_ms * 1e-3) / 1e9,
                                                 "frac_of_8TBs": tot_b / (tot_ms * 1e-3) / 8e12},
                  "kernels": {k_: {"launches_per_apply": v[0] / napp, "ms_per_apply": v[1] / napp} for k_, v in per_kernel.items()}}
        stages.update(stamp())
        json.dump(stages, open(dst + "_stage_roofline.json", "w"), indent=1)
        for r_ in table:
            print("level %d: %.3f ms  %.2f GB  %.0f GB/s (%.1f %%)" % (r_["level"], r_["ms"], r_["algorithmic_bytes"] / 1e9, r_["GBs"] or 0,
                                                                       100 * (r_["frac_of_8TBs"] or 0)), {g: round(v["ms"], 3) for g, v in r_["groups"].items()})

out = {}
f, w = one("pmc_fetch/*/*counter_collection.csv"), one("pmc_write/*/*counter_collection.csv")
if f and w:
    nf, bf = pmc(f, "FETCH_SIZE", os.path.join(src, "bench_fetch.json"))
    nw, bw = pmc(w, "WRITE_SIZE", os.path.join(src, "bench_write.json"))
    tf, tw = sum(bf.values()), sum(bw.values())
    out = {"command": "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE (separate passes) -- python3 bench.py --full --steps 3 --warmup 1 --secondary 0 --extras 0",
           "applies_profiled": [nf, nw], "unit": "KiB per 64-RHS apply (default-parameter hierarchy)",
           "FETCH_SIZE_KiB": tf, "WRITE_SIZE_KiB": tw,
           "hbm_bytes_per_apply_corrected": (2.0 * tf + tw) * 1024.0,
           "correction": "read bytes = 2 * FETCH_SIZE * 1024 (gfx950 counts 128-B requests at 64 B); "
                         "WRITE_SIZE exact (k_gather_scale: 499,709 KiB reported vs 499,709 KiB written)",
           "per_kernel_KiB": {k: {"FETCH_SIZE": bf.get(k, 0.0), "WRITE_SIZE": bw.get(k, 0.0)} for k in bf}}
    out.update(stamp())
    json.dump(out, open(dst + "_pmc_summary.json", "w"), indent=1)
print(json.dumps(out, indent=1)[:1500])
