#!/usr/bin/env python3
"""Cost of the NAT44 create path, where the port rotor runs (needs a GPU).

One MI355X and the headline's tables (1M subscribers, 1024-port blocks).
Three uplink batches of nothing but NEW flows, each timed as one launch on
empty session tables, --repeats times (the tables are wiped in between):

  distinct   one flow per subscriber: no two lanes share a rotor
  burst      --burst-subs subscribers with 64 flows each, a subscriber's
             flows in consecutive rows: the 64 lanes of a wave all
             allocate from ONE block (the worst contention a batch can hold)
  shuffled   the same flows in random row order

and, after each, the same batch again: every packet a session hit.
--near-end starts every rotor 32 ports before the end of its block, so each
burst wraps inside its wave.

Prints one JSON line per case: us per launch (median, min, max), Mpps,
verdict and counter totals, and for the burst cases how many subscribers
came out with a port outside their block or one port for two flows.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np

NOW = 1_700_000_000
FLOWS = 64


def emit(**kw):
    print(json.dumps(kw), flush=True)


def frames(idx, sports, stride):
    """64-byte UDP frames of subscribers idx (the headline's data frame)."""
    import bench
    from bng_amd.dataplane.packets import build_ipv4, ip2u32
    n = len(idx)
    t = np.frombuffer(build_ipv4(
        "aa:00:00:00:00:00", "02:00:00:00:00:01", ip2u32("10.0.0.2"),
        ip2u32("93.184.216.34"), proto=17, sport=40000, dport=53,
        payload=b"\x00" * 22), dtype=np.uint8)
    data = np.zeros((n, stride), dtype=np.uint8)
    data[:, :64] = t
    idx = idx.astype(np.uint64)
    macs = np.uint64(0xAA0000000000) + idx
    data[:, 6:12] = macs.astype(">u8").view(np.uint8).reshape(n, 8)[:, 2:]
    ips = (np.uint64(ip2u32("10.0.0.0") + 2) + idx).astype(np.uint32)
    data[:, 26:30] = ips.astype(">u4").view(np.uint8).reshape(n, 4)
    data[:, 34:36] = sports.astype(">u2").view(np.uint8).reshape(n, 2)
    assert bench  # the tables these frames match are bench.build_tables'
    return data, np.full(n, 64, dtype=np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subs", type=int, default=1_000_000)
    ap.add_argument("--burst-subs", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--near-end", action="store_true")
    args = ap.parse_args()

    import torch
    import bench
    from bng_amd.dataplane import abi
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.dataplane.packets import ip2u32

    assert torch.cuda.is_available(), "needs a GPU"
    base_log2 = max(18, (args.subs - 1).bit_length() + 1)
    l = HipLauncher("cuda:0", sub_log2=base_log2, sess_log2=base_log2 + 1,
                    eim_log2=base_log2 + 1, subnat_log2=base_log2,
                    qos_log2=base_log2, binding_log2=base_log2)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED)
    bench.build_tables(l, 0, 1, args.subs, NOW)
    if args.near_end:
        ctx = l.subctx.cpu().numpy().view(np.uint32).reshape(-1, 16)
        live = ctx[:, 0] != 0
        ctx[live, 11] = (ctx[live, 2] >> 16) - 31     # next_port = end - 31
        l.subctx.copy_(torch.from_numpy(ctx.view(np.uint8).reshape(-1))
                       .to(l.device))
    pristine = l.subctx.clone()

    def wipe():
        l.subctx.copy_(pristine)
        for t in (l.sessions, l.reverse, l.eim, l.nat_stats, l.nat_log_hdr):
            t.zero_()
        l._nat_log_ridx = 0

    rng = np.random.default_rng(1234)
    one = rng.permutation(args.subs)
    who = np.repeat(rng.choice(args.subs, args.burst_subs, replace=False),
                    FLOWS)
    sp = np.tile(40000 + np.arange(FLOWS), args.burst_subs)
    mix = rng.permutation(len(who))
    cases = [("distinct", one, np.full(len(one), 40000)),
             ("burst", who, sp), ("shuffled", who[mix], sp[mix])]

    for name, idx, sports in cases:
        data_np, lens_np = frames(idx, sports.astype(np.uint16), args.stride)
        d = torch.from_numpy(data_np).cuda()
        ln = torch.from_numpy(lens_np.view(np.int16)).cuda()
        w, wl = torch.empty_like(d), torch.empty_like(ln)
        n = len(idx)

        def launch(now_ns):
            w.copy_(d)
            wl.copy_(ln)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v, _ = l.uplink(w, wl, now_ns=now_ns, now_sec=NOW)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6, v

        create, hit = [], []
        for r in range(args.repeats + 1):             # the first is warm-up
            wipe()
            t, v = launch(NOW * 10**9)
            out = w.cpu().numpy()
            t2, _ = launch(NOW * 10**9 + 10**7)
            if r:
                create.append(t)
                hit.append(t2)
        st = l.nat_get_stats()
        rec = dict(what=name, near_end=args.near_end, packets=n,
                   subscribers=len(np.unique(idx)),
                   create_us=round(statistics.median(create), 1),
                   create_us_min=round(min(create), 1),
                   create_us_max=round(max(create), 1),
                   create_mpps=round(n / statistics.median(create), 2),
                   hit_us=round(statistics.median(hit), 1),
                   fwd=int((v == abi.FWD).sum()),
                   drop=int((v == abi.DROP).sum()),
                   sessions_created=st["sessions_created"],
                   port_exhaustion=st["port_exhaustion"])
        if name != "distinct":
            # per subscriber: the 64 ports it was given
            port = out[:, 34].astype(np.int64) << 8 | out[:, 35]
            o = np.argsort(idx, kind="stable")
            p = np.sort(port[o].reshape(-1, FLOWS), axis=1)
            start = 1024 + (idx[o].reshape(-1, FLOWS)[:, 0] % 63) * 1024
            rec["subs_with_shared_port"] = int(
                (np.diff(p, axis=1) == 0).any(axis=1).sum())
            rec["subs_with_port_outside_block"] = int(
                ((p[:, 0] < start) | (p[:, -1] > start + 1023)).sum())
        emit(**rec)


if __name__ == "__main__":
    main()
