#!/usr/bin/env python3
"""Memory-side transaction budget of the packet kernels.

For pkt_class_kernel, antispoof_kernel, qos_kernel (ingress), nat44_kernel
(egress, session hits) and uplink_pipeline_kernel, at N = 1 048 576 packets
with the benchmark's tables and batch: how many requests leave L2 for
memory per dispatch (TCC_EA0 reads, writes, atomics), how many requests L2
serves (TCC_REQ), and how long the kernel takes.  profiles/EA_BUDGET.md
sets the result against the transactions each kernel needs.

Driver (default): starts one profiler run per counter pair — each a
counters-only run of its own — and one kernel-trace run for the times;
every run executes this file with --worker.  Results: a table on stdout and
<out>/<tag>.json.

    python scripts/gpu_ea_budget.py --out prof_out/ea_budget --tag parent

Worker: builds the tables, warms up with fused uplink steps (they create
the NAT sessions every later dispatch hits), then dispatches each kernel
--reps times.  The driver keeps the last --reps dispatches of each kernel.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N = 1 << 20
SUBS = 1_000_000
NOW = 1_700_000_000
KERNELS = ["pkt_class_kernel", "antispoof_kernel", "qos_kernel",
           "nat44_kernel", "uplink_pipeline_kernel"]
# two counters per pass; the last pair exists on gfx950 builds of the
# profiler that define it and is skipped when the pass fails
PASSES = [["TCC_EA0_RDREQ_sum", "TCC_EA0_WRREQ_sum"],
          ["TCC_EA0_ATOMIC_sum", "TCC_REQ_sum"],
          ["TCC_EA0_RDREQ_32B_sum", "TCC_BUBBLE_sum"]]
OPTIONAL = {2}
PASS_TIMEOUT_S = 240


def worker(reps):
    import numpy as np
    import torch
    import bench
    from bng_amd.dataplane import abi
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.dataplane.packets import ip2u32

    l = HipLauncher("cuda:0", sub_log2=21, sess_log2=22, eim_log2=21,
                    subnat_log2=21, qos_log2=21, binding_log2=21)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED)
    bench.build_tables(l, 0, 1, SUBS, NOW)
    d_np, len_np = bench.gen_batch(N, SUBS, 0.1, 512, 1234)
    pristine = torch.from_numpy(d_np).cuda()
    lens = torch.from_numpy(len_np.view(np.int16)).cuda()
    w = torch.empty_like(pristine)
    cls = torch.empty(N, dtype=torch.uint8, device="cuda")
    ns = [NOW * 10**9]

    def tick():
        ns[0] += 10**6
        return ns[0]

    def uplink():
        w.copy_(pristine)
        l.ext.pkt_class(w, lens, cls)
        order = torch.argsort(cls, stable=True).to(torch.int32)
        l.uplink(w, lens, now_ns=tick(), now_sec=NOW, sort_by_type=True,
                 order=order)

    for _ in range(3):                   # creates the sessions
        uplink()
    torch.cuda.synchronize()
    for _ in range(reps):
        w.copy_(pristine)
        l.antispoof(w, lens, now_ns=tick())
        l.qos(w, lens, egress=False, now_ns=tick())
        l.nat44(w, lens, egress=True, now_ns=tick())
        uplink()
    torch.cuda.synchronize()
    st = l.nat_get_stats()
    print("[ea_budget] nat stats", {k: v for k, v in st.items() if v},
          flush=True)


def _col(row, *names):
    low = {k.lower(): v for k, v in row.items()}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise KeyError(f"none of {names} in {sorted(row)}")


def _kernel_of(name):
    for k in KERNELS:
        if k in name:
            return k
    return None


def _rows(out_dir, suffix):
    files = glob.glob(os.path.join(out_dir, "**", f"*{suffix}.csv"),
                      recursive=True)
    if not files:
        raise FileNotFoundError(f"no *{suffix}.csv under {out_dir}")
    for f in files:
        with open(f, newline="") as fh:
            yield from csv.DictReader(fh)


def read_counters(out_dir, reps):
    """{kernel: {counter: median over the last `reps` dispatches}}"""
    per = {}
    for r in _rows(out_dir, "counter_collection"):
        k = _kernel_of(_col(r, "Kernel_Name"))
        if k is None:
            continue
        did = int(_col(r, "Dispatch_Id"))
        c = _col(r, "Counter_Name")
        v = float(_col(r, "Counter_Value"))
        d = per.setdefault(k, {}).setdefault(c, {})
        d[did] = d.get(did, 0.0) + v     # one row per dimension instance
    return {k: {c: statistics.median([v for _, v in sorted(d.items())][-reps:])
                for c, d in cs.items()} for k, cs in per.items()}


def read_times(out_dir, reps):
    per = {}
    for r in _rows(out_dir, "kernel_trace"):
        k = _kernel_of(_col(r, "Kernel_Name"))
        if k is None:
            continue
        t0 = int(_col(r, "Start_Timestamp"))
        per.setdefault(k, []).append(
            (t0, (int(_col(r, "End_Timestamp")) - t0) / 1e3))
    return {k: statistics.median([d for _, d in sorted(v)][-reps:])
            for k, v in per.items()}


def profiler_run(out_dir, prof_args, reps):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", *prof_args, "-d", out_dir, "-o", "run", "-f", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--worker",
           "--reps", str(reps)]
    print("[ea_budget]", " ".join(cmd), flush=True)
    with open(os.path.join(out_dir, "log.txt"), "w") as log:
        return subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT,
                              timeout=PASS_TIMEOUT_S, cwd=REPO).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="prof_out/ea_budget")
    ap.add_argument("--tag", default="run")
    ap.add_argument("--no-optional", action="store_true",
                    help="skip the counter pair that may not exist")
    args = ap.parse_args()
    if args.worker:
        return worker(args.reps)

    base = os.path.join(args.out, args.tag)
    result = {k: {} for k in KERNELS}
    regex = "|".join(KERNELS)
    for i, pair in enumerate(PASSES):
        if i in OPTIONAL and args.no_optional:
            continue
        d = os.path.join(base, f"pmc{i}")
        rc = profiler_run(d, ["--pmc", *pair, "--kernel-include-regex",
                              regex], args.reps)
        if rc != 0:
            if i in OPTIONAL:
                print(f"[ea_budget] optional pass {pair} failed (rc {rc})")
                continue
            sys.exit(f"counter pass {pair} failed (rc {rc}), see {d}/log.txt")
        for k, cs in read_counters(d, args.reps).items():
            result[k].update(cs)
    d = os.path.join(base, "trace")
    rc = profiler_run(d, ["--kernel-trace"], args.reps)
    if rc != 0:
        sys.exit(f"kernel-trace pass failed (rc {rc}), see {d}/log.txt")
    for k, t in read_times(d, args.reps).items():
        result[k]["time_us"] = t

    with open(os.path.join(args.out, f"{args.tag}.json"), "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    cols = [c for p in PASSES for c in p]
    print(f"\n{args.tag}: per dispatch, N = {N} "
          f"(median of the last {args.reps})")
    print("| kernel | time us | " + " | ".join(
        c.replace("TCC_", "").replace("_sum", "") for c in cols) +
        " | EA per packet |")
    print("|---|---|" + "---|" * (len(cols) + 1))
    for k in KERNELS:
        r = result[k]
        ea = sum(r.get(c, 0.0) for c in ("TCC_EA0_RDREQ_sum",
                                         "TCC_EA0_WRREQ_sum"))
        cells = [f"{r[c] / 1e6:.3f} M" if c in r else "-" for c in cols]
        t = f"{r['time_us']:.1f}" if "time_us" in r else "-"
        print(f"| {k} | {t} | " + " | ".join(cells) + f" | {ea / N:.2f} |")


if __name__ == "__main__":
    main()
