#!/usr/bin/env python3
"""Stage bench of the PPPoE session-data fast path (needs a GPU).

For the 64-byte mix (10% DHCP) at stride 512 and for 1500-byte frames at
stride 2048, with a PPPoE share of 0, 0.5 and 1.0 of the data frames:

  * uplink:   decap + uplink pipeline on the PPPoE batch against the uplink
              pipeline alone on the batch of IPoE twins;
  * downlink: downlink pipeline + encap against the downlink pipeline alone;
  * each new kernel's own time against an ideal copy of the bytes it moves
    (read once, written once) at the measured HBM copy rate.

Every timed step starts from a fresh copy of its batch (the kernels work in
place); the copy is timed on its own and subtracted.  Prints one JSON line
per measurement.  N (packets, default 1M) and REPS from the environment.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bench
from bng_amd.dataplane import abi
from bng_amd.dataplane.launcher import HipLauncher
from bng_amd.dataplane.packets import ip2u32

N = int(os.environ.get("N", 1 << 20))
REPS = int(os.environ.get("REPS", 10))
N_SUBS = 65534                  # one PPPoE session id per subscriber
NOW = 1_700_000_000
HBM_COPY_BPS = 6.29e12          # measured float4 copy rate of the MI355X
IP_BASE = ip2u32("10.0.0.0") + 2


def timeit(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def kernel_time(prep, fn, reps=REPS):
    """Mean device time of fn alone (events), prep outside the window."""
    tot = 0.0
    for i in range(reps + 2):
        prep()
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            tot += a.elapsed_time(b)
    return tot / reps * 1e3


def sub_index(data):
    """Subscriber index of each row, from the source address (bytes 26..29
    of the IPoE frame)."""
    b = data[:, 26:30].to(torch.int64)
    ip = (b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8) | b[:, 3]
    return ip - IP_BASE


def grow(data, lens, frame_len, stride):
    """The 64-byte data frames of a batch blown up to frame_len."""
    n = data.shape[0]
    big = torch.zeros((n, stride), dtype=torch.uint8, device=data.device)
    big[:, :data.shape[1]] = data
    rows = lens == 64
    fill = (torch.arange(stride, device=data.device) * 7 & 0xFF).to(
        torch.uint8)
    big[rows, 64:frame_len] = fill[64:frame_len]
    ip_len, udp_len = frame_len - 14, frame_len - 34
    big[rows, 16], big[rows, 17] = ip_len >> 8, ip_len & 0xFF
    big[rows, 38], big[rows, 39] = udp_len >> 8, udp_len & 0xFF
    out_lens = torch.where(rows, torch.full_like(lens, frame_len), lens)
    return big, out_lens


def wrap(data, lens, frame_len, rows):
    """PPPoE twins of the selected data rows (session id = subscriber + 1)."""
    out, out_lens = data.clone(), lens.clone()
    sid = (sub_index(data[rows]) + 1).to(torch.int64)
    plen = frame_len - 14 + 2
    hdr = torch.zeros((int(rows.sum()), 10), dtype=torch.uint8,
                      device=data.device)
    hdr[:, 0], hdr[:, 1], hdr[:, 2] = 0x88, 0x64, 0x11
    hdr[:, 4], hdr[:, 5] = (sid >> 8).to(torch.uint8), \
        (sid & 0xFF).to(torch.uint8)
    hdr[:, 6], hdr[:, 7], hdr[:, 9] = plen >> 8, plen & 0xFF, 0x21
    src = data[rows]
    out[rows] = torch.cat([src[:, :12], hdr, src[:, 14:src.shape[1] - 8]], 1)
    out_lens[rows] = frame_len + 8
    return out, out_lens


class without_pppoe:
    """The launcher as it behaves with no session provisioned: uplink()
    and downlink() launch neither PPPoE kernel.  The device tables stay."""

    def __init__(self, launcher):
        self.l = launcher

    def __enter__(self):
        self.live, self.l._pppoe_live = self.l._pppoe_live, {}

    def __exit__(self, *exc):
        self.l._pppoe_live = self.live


def emit(**kw):
    print(json.dumps(kw), flush=True)


def run_shape(l, name, d_ipoe, l_ipoe, frame_len):
    stride = d_ipoe.shape[1]
    n = d_ipoe.shape[0]
    is_data = (l_ipoe == frame_len)
    idx = sub_index(d_ipoe)
    w, wl = torch.empty_like(d_ipoe), torch.empty_like(l_ipoe)
    ns = [NOW * 10**9]

    def tick():
        ns[0] += 10**6
        return ns[0]

    def fresh(src, src_lens):
        w.copy_(src)
        wl.copy_(src_lens)

    t_copy = timeit(lambda: fresh(d_ipoe, l_ipoe))
    emit(shape=name, what="copy", us=round(t_copy, 1))

    def up(src, src_lens):
        fresh(src, src_lens)
        l.uplink(w, wl, now_ns=tick(), now_sec=NOW, sort_by_type=True)

    # sessions for every subscriber: the pre-pass runs on every batch
    l.clear_pppoe_sessions()
    macs = 0xAA0000000000
    l.add_pppoe_sessions([(k + 1, macs + k, IP_BASE + k, 1492)
                          for k in range(N_SUBS)])
    for frac in (0.0, 0.5, 1.0):
        rows = is_data & ((idx % 2 == 0) if frac == 0.5 else
                          torch.full_like(is_data, frac == 1.0))
        d_p, l_p = wrap(d_ipoe, l_ipoe, frame_len, rows) if frac else \
            (d_ipoe, l_ipoe)
        with without_pppoe(l):               # uplink alone, IPoE twins
            t_alone = timeit(lambda: up(d_ipoe, l_ipoe)) - t_copy
        t_both = timeit(lambda: up(d_p, l_p)) - t_copy
        t_decap = kernel_time(lambda: fresh(d_p, l_p),
                              lambda: l.pppoe_decap(w, wl))
        moved = int(rows.sum()) * (frame_len - 14)
        ideal = 2 * moved / HBM_COPY_BPS * 1e6
        emit(shape=name, what="uplink", pppoe_frac=frac,
             uplink_alone_us=round(t_alone, 1),
             uplink_alone_mpps=round(n / t_alone, 1),
             decap_uplink_us=round(t_both, 1),
             decap_uplink_mpps=round(n / t_both, 1),
             ratio=round(t_both / t_alone, 3),
             decap_kernel_us=round(t_decap, 1),
             ideal_copy_us=round(ideal, 2),
             decap_over_ideal=round(t_decap / ideal, 1) if moved else None)

    # downlink: learn each flow's SNAT (ip, port) from one uplink pass over
    # the data rows, build the return traffic, DNAT + QoS-egress it
    fresh(d_ipoe, l_ipoe)
    with without_pppoe(l):
        l.uplink(w, wl, now_ns=tick(), now_sec=NOW, sort_by_type=True)
    torch.cuda.synchronize()
    ret = d_ipoe.clone()
    ret[:, 0:6], ret[:, 6:12] = d_ipoe[:, 6:12], d_ipoe[:, 0:6]
    ret[:, 26:30], ret[:, 30:34] = d_ipoe[:, 30:34], w[:, 26:30]
    ret[:, 34:36], ret[:, 36:38] = d_ipoe[:, 36:38], w[:, 34:36]
    ret[:, 24:26] = 0       # checksums: updated incrementally, not verified
    ret[:, 40:42] = 0
    ret, ret_lens = ret[is_data].contiguous(), l_ipoe[is_data].contiguous()
    ridx = idx[is_data]
    m = ret.shape[0]
    w2, wl2 = torch.empty_like(ret), torch.empty_like(ret_lens)

    def down():
        w2.copy_(ret)
        wl2.copy_(ret_lens)
        l.downlink(w2, wl2, now_ns=tick())

    def copy2():
        w2.copy_(ret)
        wl2.copy_(ret_lens)

    t_copy2 = timeit(copy2)
    vfwd = torch.full((m,), abi.FWD, dtype=torch.uint8, device=w2.device)
    for frac in (0.0, 0.5, 1.0):
        # sessions for the chosen share of subscribers, plus one that no
        # frame belongs to, so the post-pass runs at share 0 as well
        l.clear_pppoe_sessions()
        members = [k for k in range(N_SUBS)
                   if frac == 1.0 or (frac == 0.5 and k % 2 == 0)]
        l.add_pppoe_sessions([(k + 1, macs + k, IP_BASE + k, 1492)
                              for k in members] +
                             [(0xFFFF, macs + N_SUBS, IP_BASE + N_SUBS,
                               1492)])
        with without_pppoe(l):
            t_alone = timeit(down) - t_copy2
        t_both = timeit(down) - t_copy2
        def dnat_only():                     # what the post-pass is fed
            copy2()
            with without_pppoe(l):
                l.downlink(w2, wl2, now_ns=tick())

        t_encap = kernel_time(dnat_only,
                              lambda: l.pppoe_encap(w2, wl2, vfwd))
        hit = int(((ridx % 2 == 0) if frac == 0.5 else
                   torch.full_like(ridx, frac == 1.0, dtype=torch.bool)
                   ).sum())
        ideal = 2 * hit * (frame_len - 14) / HBM_COPY_BPS * 1e6
        emit(shape=name, what="downlink", pppoe_frac=frac, packets=m,
             encapsulated=hit, downlink_alone_us=round(t_alone, 1),
             downlink_alone_mpps=round(m / t_alone, 1),
             downlink_encap_us=round(t_both, 1),
             downlink_encap_mpps=round(m / t_both, 1),
             ratio=round(t_both / t_alone, 3),
             encap_kernel_us=round(t_encap, 1),
             ideal_copy_us=round(ideal, 2),
             encap_over_ideal=round(t_encap / ideal, 1) if hit else None)
    emit(shape=name, what="pppoe_stats", **l.pppoe_get_stats())


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    l = HipLauncher("cuda:0", sub_log2=18, sess_log2=21, eim_log2=20,
                    subnat_log2=18, qos_log2=18, binding_log2=18)
    l.set_server_config(b"\x02\x00\x00\x00\x00\x01", ip2u32("10.255.255.1"))
    l.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
               ip2u32("8.8.8.8"))
    bench.build_tables(l, 0, 1, N_SUBS + 1, NOW)
    mix_np, lens_np = bench.gen_batch(N, N_SUBS, 0.1, 512, 13)
    d64 = torch.from_numpy(mix_np).cuda()
    l64 = torch.from_numpy(lens_np.view(np.int16)).cuda()
    run_shape(l, "64B-mix/stride512", d64, l64, 64)
    d_big, l_big = grow(d64, l64, 1500, 2048)
    del d64
    run_shape(l, "1500B/stride2048", d_big, l_big, 1500)


if __name__ == "__main__":
    main()
