#!/usr/bin/env python3
"""Cost of per-subscriber traffic accounting (needs a GPU).

One MI355X, the headline's tables (1M subscribers) and its 64-byte mix (10%
DHCP), every subscriber accounted.  Prints one JSON line per measurement:

  * `bench`    — `bench.py --steps 20 --warmup 5` in a child process,
                 --bench-runs times: the headline figure and its run-to-run
                 spread, the yardstick for "no difference";
  * `uplink` / `downlink`, acct "off" — HipLauncher.uplink() / .downlink()
                 with no live entry: what they launched before accounting;
  * the same with accounting on, for a uniform choice of subscriber and for
                 a skewed one (half of the data packets from 1% of the
                 subscribers) and an extreme one (half of them from
                 --elephants subscribers), for each combining variant of
                 the commit (peel rounds 0 = none, k = bounded, -1 = until
                 done);
  * `exact`    — at this scale too, the entries' sums equal the forwarded
                 packets and bytes of a batch.

A step is a fresh copy of the batch (the kernels work in place) plus the
call; the copy is timed alone and subtracted.  Each figure is the median of
--repeats runs of --steps steps after --warmup; min and max are the spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np

NOW = 1_700_000_000


def emit(**kw):
    print(json.dumps(kw), flush=True)


def run_bench(runs):
    vals = []
    for i in range(runs):
        p = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", "20", "--warmup", "5"],
            capture_output=True, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            emit(what="bench", run=i, error=p.stderr[-300:])
            raise SystemExit(1)
        vals.append(json.loads(line[-1])["value"])
        emit(what="bench", run=i, mpps=vals[-1])
    if vals:
        emit(what="bench_spread", runs=runs, median=statistics.median(vals),
             min=min(vals), max=max(vals),
             spread_pct=round(100 * (max(vals) - min(vals)) /
                              statistics.median(vals), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--variants", default="0,1,2,4,8,-1")
    ap.add_argument("--elephants", type=int, default=16)
    args = ap.parse_args()
    variants = [int(v) for v in args.variants.split(",")]

    # the children first: they want the whole device
    run_bench(args.bench_runs)

    import torch
    import bench
    from bng_amd.dataplane import abi
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.dataplane.packets import ip2u32

    assert torch.cuda.is_available(), "needs a GPU"
    ip_base = ip2u32("10.0.0.0") + 2
    base_log2 = max(18, (args.subs - 1).bit_length() + 1)
    l = HipLauncher("cuda:0", sub_log2=base_log2, sess_log2=base_log2 + 1,
                    eim_log2=base_log2, subnat_log2=base_log2,
                    qos_log2=base_log2, binding_log2=base_log2,
                    acct_log2=base_log2)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED)
    bench.build_tables(l, 0, 1, args.subs, NOW)
    n = args.batch
    ns = [NOW * 10**9]

    def tick():
        # 20 ms a step: an elephant's 1 Gbps bucket refills what its ~30k
        # packets of a batch took, so the verdicts stay FWD
        ns[0] += 2 * 10**7
        return ns[0]

    def figure(fn):
        """us per step: median, min, max over the repeats."""
        ts = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / args.steps * 1e6)
        return statistics.median(ts), min(ts), max(ts)

    def batch_for(mix):
        data_np, lens_np = bench.gen_batch(n, args.subs, 0.1, 512, seed=1234)
        if mix != "uniform":
            # half of the data packets from a hot set: the first 1% of the
            # subscribers, or --elephants of them (the case where one
            # subscriber owns many lanes of a wave)
            rng = np.random.default_rng(99)
            rows = np.nonzero(lens_np == 64)[0]
            hot = max(1, args.subs // 100) if mix == "skewed" \
                else args.elephants
            idx = np.where(rng.random(len(rows)) < 0.5,
                           rng.integers(0, hot, len(rows)),
                           rng.integers(0, args.subs, len(rows))
                           ).astype(np.uint64)
            macs = np.uint64(0xAA0000000000) + idx
            data_np[rows[:, None], np.arange(6, 12)] = \
                macs.astype(">u8").view(np.uint8).reshape(-1, 8)[:, 2:]
            data_np[rows[:, None], np.arange(26, 30)] = \
                (np.uint64(ip_base) + idx).astype(">u4").view(np.uint8) \
                .reshape(-1, 4)
            data_np[rows[:, None], np.arange(34, 36)] = \
                (40000 + (idx & np.uint64(0x3F))).astype(">u2") \
                .view(np.uint8).reshape(-1, 2)
        d = torch.from_numpy(data_np).cuda()
        ln = torch.from_numpy(lens_np.view(np.int16)).cuda()
        cls = torch.empty(n, dtype=torch.uint8, device=d.device)
        l.ext.pkt_class(d, ln, cls)
        order = torch.argsort(cls, stable=True).to(torch.int32)
        return d, ln, order

    mixes = {}
    for mix in ("uniform", "skewed", "elephants"):
        d, ln, order = batch_for(mix)
        w, wl = torch.empty_like(d), torch.empty_like(ln)

        def fresh(d=d, ln=ln, w=w, wl=wl):
            w.copy_(d)
            wl.copy_(ln)

        def up(d=d, ln=ln, w=w, wl=wl, order=order):
            w.copy_(d)
            wl.copy_(ln)
            return l.uplink(w, wl, now_ns=tick(), now_sec=NOW, order=order)

        # return traffic against the sessions one uplink pass creates
        v, _ = up()
        torch.cuda.synchronize()
        keep = (ln == 64) & (v == abi.FWD)
        ret = d.clone()
        ret[:, 0:6], ret[:, 6:12] = d[:, 6:12], d[:, 0:6]
        ret[:, 26:30], ret[:, 30:34] = d[:, 30:34], w[:, 26:30]
        ret[:, 34:36], ret[:, 36:38] = d[:, 36:38], w[:, 34:36]
        ret[:, 24:26] = 0     # checksums: updated incrementally, not verified
        ret[:, 40:42] = 0
        ret, rl = ret[keep].contiguous(), ln[keep].contiguous()
        w2, wl2 = torch.empty_like(ret), torch.empty_like(rl)

        def fresh2(ret=ret, rl=rl, w2=w2, wl2=wl2):
            w2.copy_(ret)
            wl2.copy_(rl)

        def down(ret=ret, rl=rl, w2=w2, wl2=wl2):
            w2.copy_(ret)
            wl2.copy_(rl)
            return l.downlink(w2, wl2, now_ns=tick())

        mixes[mix] = dict(up=up, down=down, fresh=fresh, fresh2=fresh2,
                          m=ret.shape[0], n_data=int((ln == 64).sum()))

    def measure(acct, rounds=None):
        for mix, b in mixes.items():
            for what, fn, cp, pk in (("uplink", b["up"], b["fresh"], n),
                                     ("downlink", b["down"], b["fresh2"],
                                      b["m"])):
                c = figure(cp)[0]
                med, lo, hi = (t - c for t in figure(fn))
                emit(what=what, mix=mix, acct=acct, rounds=rounds,
                     packets=pk, copy_us=round(c, 1), us=round(med, 1),
                     us_min=round(lo, 1), us_max=round(hi, 1),
                     mpps=round(pk / med, 1),
                     mpps_min=round(pk / hi, 1), mpps_max=round(pk / lo, 1))

    assert l.acct is None and l.acct_count == 0
    measure("off")
    assert l.acct_launches == {"resolve": 0, "commit": 0, "downlink": 0}

    ips = (np.uint64(ip_base) + np.arange(args.subs, dtype=np.uint64))
    t0 = time.perf_counter()
    l.acct_add(ips.tolist())
    emit(what="acct_add", entries=l.acct_count,
         seconds=round(time.perf_counter() - t0, 2))
    default = l.ext.get_acct_combine()
    for r in variants:
        l.ext.set_acct_combine(r)
        measure("on", r)
    l.ext.set_acct_combine(default)

    # exactness at scale, each variant: one uplink and one downlink batch
    # from zeroed entries
    for r in variants:
        l.ext.set_acct_combine(r)
        for mix, b in mixes.items():
            l.acct_add(ips.tolist(), reset=True)
            v, ol = b["up"]()
            vd = b["down"]()
            e = l.acct_export()
            fwd_up = (v == abi.FWD)
            want_up = int(fwd_up.sum())
            want_up_b = int((ol.to(torch.int64) & 0xFFFF)[fwd_up].sum())
            want_dn = int((vd == abi.FWD).sum())
            got = {k: int(e[k].sum()) for k in
                   ("up_pkts", "up_bytes", "down_pkts", "down_bytes",
                    "up_drop_pkts", "down_drop_pkts")}
            # every subscriber is accounted and only data frames forward
            ok = (got["up_pkts"] == want_up and
                  got["up_bytes"] == want_up_b and
                  got["down_pkts"] == want_dn and
                  got["down_bytes"] == 64 * want_dn and
                  got["up_drop_pkts"] <= int((v == abi.DROP).sum()) and
                  got["down_drop_pkts"] <= int((vd == abi.DROP).sum()))
            emit(what="exact", mix=mix, rounds=r, ok=ok, fwd_up=want_up,
                 fwd_up_bytes=want_up_b, fwd_down=want_dn, **got)
            assert ok, "entry sums differ from the verdicts"
    l.ext.set_acct_combine(default)


if __name__ == "__main__":
    main()
