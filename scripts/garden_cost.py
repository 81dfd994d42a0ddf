#!/usr/bin/env python3
"""Cost of the walled-garden gate on the uplink (needs a GPU).

One MI355X, the headline's tables (1M subscribers) and its 1M-packet batch
(64-byte mix, 10% DHCP).  Times HipLauncher.uplink() with the garden empty
(the baseline: no gate kernel is launched) and with 0 %, 1 % and 100 % of
the subscribers quarantined.  "0 %" is one live entry that no packet of the
batch matches: the gate kernel runs and decides nothing.  The batch's data
frames go to a destination outside the allow-list, so a quarantined
subscriber's frames leave the gate with DROP and never enter the pipeline —
at 100 % the pipeline has only the DHCP tenth left to do.  A last run puts
that destination on the allow-list: the same frames leave with ALLOW (FWD).

Prints one JSON line per measurement: us per batch (median, min, max of
--repeats runs of --steps steps after --warmup, the batch copy timed alone
and subtracted), the ratio to the baseline and the added us.
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch
    import bench
    from bng_amd.dataplane import abi
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.dataplane.packets import ip2u32

    assert torch.cuda.is_available(), "needs a GPU"
    ip_base = ip2u32("10.0.0.0") + 2
    mac_base = 0xAA0000000000
    base_log2 = max(18, (args.subs - 1).bit_length() + 1)
    l = HipLauncher("cuda:0", sub_log2=base_log2, sess_log2=base_log2 + 1,
                    eim_log2=base_log2, subnat_log2=base_log2,
                    qos_log2=base_log2, binding_log2=base_log2,
                    wg_log2=base_log2)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED)
    bench.build_tables(l, 0, 1, args.subs, NOW)
    portal, dns = ip2u32("10.255.255.1"), ip2u32("10.255.255.53")
    garden = [(dns, 53, 17), (dns, 53, 6), (portal, 8080, 6)]
    l.wg_set_config(garden)

    n = args.batch
    data_np, lens_np = bench.gen_batch(n, args.subs, 0.1, 512, seed=1234)
    d = torch.from_numpy(data_np).cuda()
    ln = torch.from_numpy(lens_np.view(np.int16)).cuda()
    cls = torch.empty(n, dtype=torch.uint8, device=d.device)
    l.ext.pkt_class(d, ln, cls)
    order = torch.argsort(cls, stable=True).to(torch.int32)
    w, wl = torch.empty_like(d), torch.empty_like(ln)
    ns = [NOW * 10**9]

    def fresh():
        w.copy_(d)
        wl.copy_(ln)

    def up():
        fresh()
        ns[0] += 2 * 10**7
        return l.uplink(w, wl, now_ns=ns[0], now_sec=NOW, order=order)

    def figure(fn):
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

    base = [None]

    def measure(label):
        c = figure(fresh)[0]
        med, lo, hi = (t - c for t in figure(up))
        v, _ = up()
        gates = np.bincount(l.last_wg_gate.cpu().numpy(), minlength=6) \
            if l.wg_count else np.zeros(6, dtype=np.int64)
        if base[0] is None:
            base[0] = med
        emit(what="uplink", garden=label, entries=l.wg_count, packets=n,
             copy_us=round(c, 1), us=round(med, 1), us_min=round(lo, 1),
             us_max=round(hi, 1), mpps=round(n / med, 1),
             ratio=round(med / base[0], 3), added_us=round(med - base[0], 1),
             gated=int(gates[1:].sum()),
             fwd=int((v == abi.FWD).sum()), drop=int((v == abi.DROP).sum()),
             wg_launches=l.wg_launches["uplink"])

    assert l.wg is None and l.wg_count == 0
    measure("empty")
    assert l.wg_launches == {"uplink": 0, "downlink": 0}

    # one live entry nobody in the batch matches: the gate runs, decides
    # nothing
    stranger = ip2u32("192.0.2.1")
    l.wg_set([(stranger, 1, abi.WG_WALLED)])
    measure("0%")
    l.wg_remove([stranger])

    def entries(idx):
        return list(zip((ip_base + idx).tolist(), (mac_base + idx).tolist(),
                        [abi.WG_WALLED] * len(idx)))

    one = np.arange(0, args.subs, 100, dtype=np.int64)
    t0 = time.perf_counter()
    l.wg_set(entries(one))
    emit(what="wg_set", entries=l.wg_count,
         seconds=round(time.perf_counter() - t0, 2))
    measure("1%")

    rest = np.setdiff1d(np.arange(args.subs, dtype=np.int64), one)
    t0 = time.perf_counter()
    l.wg_set(entries(rest))
    emit(what="wg_set", entries=l.wg_count,
         seconds=round(time.perf_counter() - t0, 2))
    measure("100%")

    # the same garden with the batch's destination on the allow-list: every
    # data frame is forwarded at the gate (ALLOW) instead of dropped
    l.wg_set_config(garden + [(ip2u32("93.184.216.34"), 53, 17)])
    measure("100%, allow-listed")
    emit(what="wg_stats", **l.wg_get_stats())


if __name__ == "__main__":
    main()
