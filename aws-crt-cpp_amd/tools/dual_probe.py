"""The fused CRC32 + CRC32C call against the two single calls it replaces, on BASELINE config 3's
shape (16 x 256 MiB) and on 16 x 64 MiB.

    python aws-crt-cpp_amd/tools/dual_probe.py [--shapes 16x256,16x64] [--reps 9] [--warm-ms 120]
                                                [--session NAME] [--out profiles/r07/dual]

Per shape, in a child process of its own under a time limit (a shape that fails or runs out of time
ends the probe: nothing more is started on the device):
  * the three calls -- aws_crt_amd_crc32_dual_strided, aws_crt_amd_checksum_strided(CRC32) and
    (CRC32C) -- are warmed up, and the fused results are checked against the two single calls;
  * a sustained warm-up runs the three interleaved for --warm-ms, so the timed launches of all three
    sit in the same power regime;
  * --reps rounds of (fused, CRC32, CRC32C), back to back on one stream, each launch stamped with
    the engine's own dispatch events (time_next_launch: the fused call from its scan's start to its
    finish pass's end).
The record (one JSON file, also printed) holds the medians and min-max per call, the fused call's
payload fraction of 8 TB/s with the bytes counted once, the ratio fused / (CRC32 + CRC32C), and
`wins`: the fused median is below the sum of the single medians by more than that sum's own min-max
spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PEAK = 8.0e12
STEP_LIMIT_S = 300


def measure(count, mib, reps, warm_ms):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    import aws_crt_amd as eng

    eng.init()
    dev = torch.device("cuda", 0)
    L = mib << 20
    data = torch.empty(count * L, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0xD0A1)
    for i in range(count):
        data[i * L:(i + 1) * L].copy_(torch.randint(0, 256, (L,), dtype=torch.uint8, device=dev, generator=g))
    st = torch.cuda.Stream()
    o2 = torch.empty((count, 2), dtype=torch.int32, device=dev)
    o32 = torch.empty(count, dtype=torch.int32, device=dev)
    o32c = torch.empty(count, dtype=torch.int32, device=dev)
    calls = {
        "fused": lambda: eng.checksum_dual_strided(data, L, L, count, out=o2, stream=st),
        "crc32": lambda: eng.checksum_strided(eng.CRC32, data, L, L, count, out=o32, stream=st),
        "crc32c": lambda: eng.checksum_strided(eng.CRC32C, data, L, L, count, out=o32c, stream=st),
    }
    before = eng.dual_fused_launches()
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    assert eng.dual_fused_launches() == before + 1, "the fused kernel did not serve the call"
    same = bool(torch.equal(o2[:, 0], o32) and torch.equal(o2[:, 1], o32c))
    if not same:
        raise SystemExit("fused results differ from the single calls")
    t0 = time.perf_counter()
    rounds = 0
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        for f in calls.values():
            f()
        rounds += 1
        if rounds % 4 == 0:
            torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for k in calls}
    for r in range(reps):
        for k, f in calls.items():
            for e in ev[k][r]:
                e.record(st)  # creates the events; the launch below re-stamps them
            eng.time_next_launch(*ev[k][r])
            f()
    torch.cuda.synchronize()
    us = {k: [eng.event_ms(a, b) * 1e3 for a, b in ev[k]] for k in calls}
    same_after = bool(torch.equal(o2[:, 0], o32) and torch.equal(o2[:, 1], o32c))
    nbytes = count * L
    rec = {"shape": f"{count}x{mib}MiB", "bytes": nbytes, "reps": reps, "warm_ms": warm_ms, "warm_rounds": rounds,
           "results_equal": same and same_after, "us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
    for k, v in us.items():
        med = statistics.median(v)
        rec[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "payload_frac_of_8TBps": round(nbytes / (med * 1e-6) / PEAK, 4)}
    s_med = rec["crc32"]["median_us"] + rec["crc32c"]["median_us"]
    s_min = rec["crc32"]["min_us"] + rec["crc32c"]["min_us"]
    s_max = rec["crc32"]["max_us"] + rec["crc32c"]["max_us"]
    rec["singles_sum"] = {"median_us": round(s_med, 2), "min_us": round(s_min, 2), "max_us": round(s_max, 2),
                          "payload_frac_of_8TBps": round(nbytes / (s_med * 1e-6) / PEAK, 4)}
    rec["ratio_fused_over_singles"] = round(rec["fused"]["median_us"] / s_med, 4)
    rec["gap_us"] = round(s_med - rec["fused"]["median_us"], 2)
    rec["singles_spread_us"] = round(s_max - s_min, 2)
    rec["wins"] = bool(rec["fused"]["median_us"] < s_med and rec["gap_us"] > rec["singles_spread_us"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x256,16x64", help="COUNTxMiB, comma separated")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm-ms", type=float, default=120.0)
    ap.add_argument("--session", default="session")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "r07", "dual"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    if a.child:
        count, mib = (int(x) for x in a.child.split("x"))
        print("RECORD " + json.dumps(measure(count, mib, a.reps, a.warm_ms)), flush=True)
        return 0
    record = {"tool": "dual_probe", "session": a.session, "shapes": []}
    rc = 0
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--warm-ms", str(a.warm_ms)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            record["shapes"].append({"shape": shape, "error": f"no result within {STEP_LIMIT_S} s"})
            rc = 1
            break  # nothing more is started on the device
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")), None)
        if r.returncode != 0 or line is None:
            record["shapes"].append({"shape": shape, "error": f"exit {r.returncode}", "stderr": r.stderr[-2000:]})
            rc = 1
            break
        record["shapes"].append(json.loads(line[len("RECORD "):]))
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"{a.session}.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))
    return rc


if __name__ == "__main__":
    sys.exit(main())
