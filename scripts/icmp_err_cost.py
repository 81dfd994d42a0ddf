#!/usr/bin/env python3
"""Cost of inbound ICMP-error translation on the downlink (needs a GPU).

One MI355X, the headline's tables and a 1M-packet downlink batch over live
NAT sessions: an uplink batch opens the flows, the downlink batch is one
64-byte UDP reply per row to the sessions it left (as bench.py --full
does).  Times HipLauncher.downlink() in one of three modes, one per
process so each runs under a time limit of its own:

  off   NAT_FLAG_ICMP_ERR clear (the only mode a build without the flag has)
  on0   flag set, no error frame in the batch
  on1   flag set, 1 % of the rows replaced by a Destination Unreachable
        (port unreachable) quoting the flow's translated datagram

Prints one JSON line: us per batch (median, min, max of --repeats runs of
--steps steps after --warmup, the batch copy timed alone and subtracted),
Mpps, and the NAT counters one batch moved.
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


def fold(s):
    s = (s & 0xFFFF) + (s >> 16)
    return (s & 0xFFFF) + (s >> 16)


def csum_rows(rows, lo, hi):
    """Ones-complement checksum over bytes lo..hi of every row."""
    w = rows[:, lo:hi].astype(np.uint64)
    s = (w[:, 0::2] << 8).sum(axis=1) + w[:, 1::2].sum(axis=1)
    return (0xFFFF - fold(fold(s))).astype(np.uint16)


def put16(rows, off, v):
    rows[:, off] = v >> 8
    rows[:, off + 1] = v & 0xFF


def error_rows(replies):
    """A port-unreachable per reply row: what the subscriber's peer would
    send about the datagram the NAT translated (70 bytes)."""
    n = len(replies)
    e = np.zeros((n, replies.shape[1]), dtype=np.uint8)
    e[:, :14] = replies[:, :14]
    e[:, 14:34] = np.frombuffer(bytes.fromhex(
        "45c00038424200004001000000000000" "00000000"), dtype=np.uint8)
    e[:, 26:30] = replies[:, 26:30]          # from the remote end
    e[:, 30:34] = replies[:, 30:34]          # to the public address
    e[:, 34] = 3
    e[:, 35] = 3
    # the quote: public address:port -> remote address:port, UDP
    e[:, 42:62] = np.frombuffer(bytes.fromhex(
        "4500002e123400003f11000000000000" "00000000"), dtype=np.uint8)
    e[:, 54:58] = replies[:, 30:34]
    e[:, 58:62] = replies[:, 26:30]
    e[:, 62:64] = replies[:, 36:38]          # source port: the NAT's
    e[:, 64:66] = replies[:, 34:36]
    e[:, 66:68] = (0, 26)
    put16(e, 52, csum_rows(e, 42, 62))
    put16(e, 36, csum_rows(e, 34, 70))
    put16(e, 24, csum_rows(e, 14, 34))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("off", "on0", "on1"), default="off")
    ap.add_argument("--subs", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch
    import bench
    from bng_amd.dataplane import abi
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.dataplane.packets import build_ipv4, ip2u32

    assert torch.cuda.is_available(), "needs a GPU"
    flag = getattr(abi, "NAT_FLAG_ICMP_ERR", None)
    if args.mode != "off" and flag is None:
        sys.exit("this build has no NAT_FLAG_ICMP_ERR: only --mode off")
    base_log2 = max(18, (args.subs - 1).bit_length() + 1)
    l = HipLauncher("cuda:0", sub_log2=base_log2, sess_log2=base_log2 + 1,
                    eim_log2=base_log2, subnat_log2=base_log2,
                    qos_log2=base_log2, binding_log2=base_log2)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    l.set_antispoof_config(default_mode=abi.AS_DISABLED)
    bench.build_tables(l, 0, 1, args.subs, NOW)
    l.set_nat_config(flags=abi.NAT_FLAG_EIM |
                     (flag if args.mode != "off" else 0))

    # open the flows
    n = args.batch
    data_np, lens_np = bench.gen_batch(n, args.subs, 0.0, 512, seed=1234)
    d = torch.from_numpy(data_np).cuda()
    ln = torch.from_numpy(lens_np.view(np.int16)).cuda()
    l.uplink(d, ln, now_ns=NOW * 10**9, now_sec=NOW)
    recs = l.export_nat_sessions()
    assert len(recs) >= 1000, len(recs)
    del d, ln

    # one reply per row, round robin over the sessions
    sel = recs[np.arange(n) % len(recs)]
    ret = np.zeros((n, 512), dtype=np.uint8)
    ret[:, :64] = np.frombuffer(build_ipv4(
        "02:00:00:00:00:01", "aa:00:00:00:00:00", ip2u32("93.184.216.34"),
        ip2u32("203.0.113.1"), proto=17, sport=53, dport=1024,
        payload=b"\x00" * 22), dtype=np.uint8)
    for off, field, kind in ((26, "dst_ip", ">u4"), (30, "nat_ip", ">u4"),
                             (34, "dst_port", ">u2"), (36, "nat_port", ">u2")):
        w = int(kind[2])
        ret[:, off:off + w] = sel[field].astype(kind).view(np.uint8) \
            .reshape(-1, w)
    rlens = np.full(n, 64, dtype=np.uint16)
    if args.mode == "on1":
        rows = np.arange(0, n, 100)
        ret[rows] = error_rows(ret[rows])
        rlens[rows] = 70
    dl = torch.from_numpy(ret).cuda()
    dll = torch.from_numpy(rlens.view(np.int16)).cuda()
    w = torch.empty_like(dl)
    ns = [NOW * 10**9]

    def fresh():
        w.copy_(dl)

    def down():
        fresh()
        ns[0] += 10**6
        return l.downlink(w, dll, now_ns=ns[0])

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

    c = figure(fresh)[0]
    med, lo, hi = (t - c for t in figure(down))
    before = l.nat_get_stats()
    v = down()
    after = l.nat_get_stats()
    print(json.dumps(dict(
        what="downlink", label=args.label, mode=args.mode, packets=n,
        sessions=len(recs), copy_us=round(c, 1), us=round(med, 1),
        us_min=round(lo, 1), us_max=round(hi, 1), mpps=round(n / med, 1),
        fwd=int((v == abi.FWD).sum()),
        moved={k: after[k] - before[k] for k in after
               if after[k] != before[k]})), flush=True)


if __name__ == "__main__":
    main()
