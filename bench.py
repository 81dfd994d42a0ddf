#!/usr/bin/env python3
"""bench.py — flagship BNG dataplane benchmark (driver contract).

Measures the BASELINE.json headline: Mpps + p50 DHCP OFFER latency on a
64B IPv4 mix with a 1M-subscriber table, at 1..8 MI355X GPUs.

One step = ingest one fixed-size synthetic batch per GPU (restore from
pristine = the RX-DMA analog), steer mis-delivered packets to their
owning shard via RCCL all-to-all over xGMI (world>1), and run the fused
uplink pipeline (DHCP fast path for UDP:67; antispoof -> NAT44 SNAT ->
QoS for data packets) on the local shard's HBM tables.  Weak scaling:
per-GPU injected batch is fixed as N grows.

Arrival model at world>1 mirrors the reference's NIC edge: RSS steers
each data flow to the core owning its subscriber (per-core XDP never
ships packets cross-core, loader.go RSS assumption), so data packets
arrive at their IP-shard owner; DHCP broadcasts cannot be RSS-steered by
subscriber MAC and arrive anywhere — the dhcp_frac slice crosses xGMI to
its MAC-shard owner each step.  --steer-all instead routes EVERY packet
through the all-to-all (full-shuffle stress mode).  RX copy, steering
exchange and type-sort for batch k+1 all overlap batch k's pipeline
kernel on a second HIP stream.

Traffic mix (configurable): 90% 64-byte UDP IPv4 data packets from
subscriber IPs (SNAT + QoS + antispoof path), 10% DHCP DISCOVER/REQUEST
(fast-path OFFER/ACK built in place).  Tables: 1M subscribers / NAT
blocks / QoS buckets / antispoof bindings, random-init, sharded by the
MAC/IP hashring when N>1.

A plain run sets up, warms up, times --steps steps and prints the result
line (Mpps, ms_per_step).  --full adds the secondary phases after the
timed steps: launched-batch DHCP OFFER p50/p99, the downlink return
path, persistent-service latency and the host-boundary conveyor; without
it their result fields are null.  --dump-outputs DIR writes what the
last timed step returned as .npy files (see dump_outputs).

vs_baseline: the reference's published Mpps figure on this metric is the
XDP single-core packet rate it cites (24 Mpps/core, BASELINE.md "XDP
single-core packet rate"); its DHCP-specific ceiling is 1-2 Mpps
(BASELINE.md "DHCP packet-rate ceiling").  We divide by 24.0.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
import sys
sys.path.insert(0, REPO)

from bng_amd.dataplane import abi
from bng_amd.dataplane.packets import build_dhcp_request, build_ipv4, ip2u32

BASELINE_MPPS = 24.0

MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64_np(x: np.ndarray) -> np.ndarray:
    """Vectorized splitmix64 finalizer, must match abi.mix64."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & MASK64
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & MASK64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & MASK64
        return z ^ (z >> np.uint64(31))


def build_tables(launcher, rank: int, world: int, n_subs: int, now_sec: int):
    """Bulk-populate subscriber/NAT/QoS/binding tables for this shard."""
    import torch
    idx = np.arange(n_subs, dtype=np.uint64)
    macs = np.uint64(0xAA0000000000) + idx
    ips = (np.uint64(ip2u32("10.0.0.0") + 2) + idx).astype(np.uint64)

    mac_owner = mix64_np(macs) % np.uint64(world)
    ip_owner = mix64_np(ips) % np.uint64(world)

    dev = launcher.device

    def to_dev_u8(arr):
        return torch.from_numpy(arr.view(np.uint8)).to(dev).flatten()

    # subscriber_pools entries (MAC-owned shard)
    sel = np.nonzero(mac_owner == rank)[0]
    sub = np.zeros(len(sel), dtype=[("key", "<u8"), ("pool", "<u4"),
                                    ("ip", "<u4"), ("lease", "<u8"),
                                    ("vlan", "<u2"), ("cc", "u1"),
                                    ("fl", "u1"), ("pad", "<u4")])
    sub["key"] = macs[sel]
    sub["pool"] = 1
    sub["ip"] = ips[sel].astype(np.uint32)
    sub["lease"] = now_sec + 86400
    rc = torch.zeros(len(sel), dtype=torch.int32, device=dev)
    launcher.ext.sub_upsert(launcher.subs, to_dev_u8(sub), rc)
    n_bad = int((rc != 0).sum().item())
    assert n_bad == 0, f"{n_bad} subscriber upserts failed (table too full)"

    # merged subscriber context (IP-owned shard): NAT port block +
    # ingress QoS bucket (1 Gbps / 4 MB burst => pass) in one 64-B entry
    sel = np.nonzero(ip_owner == rank)[0]
    pub_base = ip2u32("203.0.113.0")
    ctx = np.zeros(len(sel), dtype=[("key_ip", "<u4"), ("pub", "<u4"),
                                    ("ps", "<u2"), ("pe", "<u2"),
                                    ("qv", "u1"), ("nv", "u1"),
                                    ("prio", "u1"), ("fl", "u1"),
                                    ("rate", "<u8"), ("tokens", "<i8"),
                                    ("last", "<u8"), ("burst", "<u4"),
                                    ("np", "<u4"), ("sid", "<u4"),
                                    ("sa", "<u4"), ("st", "<u4"),
                                    ("pad", "<u4")])
    ctx["key_ip"] = ips[sel].astype(np.uint32)
    ctx["sid"] = sel.astype(np.uint32)
    ctx["pub"] = pub_base + (sel % 250).astype(np.uint32)
    starts = (1024 + (sel % 63) * 1024).astype(np.uint16)
    ctx["ps"] = starts
    ctx["pe"] = starts + 1023
    ctx["np"] = starts
    ctx["nv"] = 1
    ctx["qv"] = 1
    ctx["rate"] = 10**9
    ctx["tokens"] = 4 << 20
    ctx["burst"] = 4 << 20
    ctx["last"] = now_sec * 10**9
    rc = torch.zeros(len(sel), dtype=torch.int32, device=dev)
    launcher.ext.subctx_upsert(launcher.subctx, to_dev_u8(ctx),
                               abi.CTX_SET_NAT | abi.CTX_SET_QOS, rc)
    assert int((rc != 0).sum().item()) == 0

    # antispoof strict bindings (packets arrive by IP shard, keyed by MAC;
    # mode strict: src ip must equal the bound ip)
    bind = np.zeros(len(sel), dtype=[("mac", "<u8"), ("ip", "<u4"),
                                     ("v4", "u1"), ("v6", "u1"),
                                     ("mode", "u1"), ("pad", "u1"),
                                     ("v6a", "16u1")])
    bind["mac"] = macs[sel]
    bind["ip"] = ips[sel].astype(np.uint32)
    bind["v4"] = 1
    bind["mode"] = abi.AS_STRICT
    rc = torch.zeros(len(sel), dtype=torch.int32, device=dev)
    launcher.ext.binding_upsert(launcher.bindings, to_dev_u8(bind), rc)
    assert int((rc != 0).sum().item()) == 0


def gen_batch(n_pkts: int, n_subs: int, dhcp_frac: float, stride: int,
              seed: int, rank: int = 0, world: int = 1,
              steer_all: bool = False):
    """Vectorized synthetic batch: [n,stride] uint8 + lens int16.

    world>1 models the NIC edge the reference also relies on: RSS steers
    each data flow to the core/GPU owning its subscriber (per-core XDP
    never ships packets cross-core), so data-packet subscribers are drawn
    from THIS rank's IP shard.  DHCP broadcasts cannot be RSS-steered to
    the MAC owner and arrive anywhere — drawn from ALL subscribers; the
    xGMI all-to-all steers those strays.  steer_all=True instead draws
    everything uniformly (the full-shuffle stress mode)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_subs, size=n_pkts, dtype=np.uint64)
    is_dhcp = rng.random(n_pkts) < dhcp_frac
    if world > 1 and not steer_all:
        all_ips = (np.uint64(ip2u32("10.0.0.0") + 2) +
                   np.arange(n_subs, dtype=np.uint64))
        local = np.nonzero(mix64_np(all_ips) % np.uint64(world) ==
                           np.uint64(rank))[0].astype(np.uint64)
        idx = np.where(is_dhcp, idx,
                       local[rng.integers(0, len(local), size=n_pkts)])

    data = np.zeros((n_pkts, stride), dtype=np.uint8)
    lens = np.zeros(n_pkts, dtype=np.uint16)

    # templates
    udp_t = np.frombuffer(build_ipv4(
        "aa:00:00:00:00:00", "02:00:00:00:00:01", ip2u32("10.0.0.2"),
        ip2u32("93.184.216.34"), proto=17, sport=40000, dport=53,
        payload=b"\x00" * 22), dtype=np.uint8)          # 64 bytes
    assert len(udp_t) == 64
    dhcp_t = np.frombuffer(build_dhcp_request(
        "aa:00:00:00:00:00", 1, xid=1), dtype=np.uint8)
    dhcp_req_t = np.frombuffer(build_dhcp_request(
        "aa:00:00:00:00:00", 3, xid=1), dtype=np.uint8)

    macs = (np.uint64(0xAA0000000000) + idx)
    mac_b = macs.astype(">u8").view(np.uint8).reshape(n_pkts, 8)[:, 2:]
    ips = (np.uint64(ip2u32("10.0.0.0") + 2) + idx).astype(np.uint32)
    ip_b = ips.astype(">u4").view(np.uint8).reshape(n_pkts, 4)
    sports = (40000 + (idx & np.uint64(0x3F))).astype(np.uint16)
    sport_b = sports.astype(">u2").view(np.uint8).reshape(n_pkts, 2)

    d = ~is_dhcp
    nd = int(d.sum())
    if nd:
        data[d, :64] = udp_t
        data[np.nonzero(d)[0][:, None], np.arange(6, 12)] = mac_b[d]
        data[np.nonzero(d)[0][:, None], np.arange(26, 30)] = ip_b[d]
        data[np.nonzero(d)[0][:, None], np.arange(34, 36)] = sport_b[d]
        lens[d] = 64
    h = is_dhcp
    nh = int(h.sum())
    if nh:
        half = rng.random(n_pkts) < 0.5
        t1 = h & half
        t2 = h & ~half
        for mask, t in ((t1, dhcp_t), (t2, dhcp_req_t)):
            k = int(mask.sum())
            if not k:
                continue
            rows = np.nonzero(mask)[0]
            data[rows, :len(t)] = t
            data[rows[:, None], np.arange(6, 12)] = mac_b[mask]      # eth src
            data[rows[:, None], np.arange(70, 76)] = mac_b[mask]     # chaddr
            lens[mask] = len(t)
    return data, lens


def log(rank, msg):
    if rank == 0:
        print(msg, file=sys.stderr, flush=True)


def build_cell_map(lens_np, stride):
    """NIC-RX-ring analog layout: each frame occupies ceil(len/64)
    64-byte cells in a contiguous pinned buffer; DHCP-sized frames
    (len>64) carry a 64-byte growth budget so the in-place OFFER/ACK
    (fixed option set, always < input+64) never spills its cells.
    Returns (n_cells_total, slot_cell_idx[int64 C]) where
    slot_cell_idx[c] is the destination 64-B cell inside the
    [n, stride] slot layout."""
    cells_per_slot = stride // 64
    grown = np.minimum((lens_np.astype(np.int64) + 64 + 63) // 64,
                       cells_per_slot)
    cells = np.where(lens_np > 64, grown,
                     (lens_np.astype(np.int64) + 63) // 64)
    off = np.zeros(len(lens_np) + 1, dtype=np.int64)
    np.cumsum(cells, out=off[1:])
    C = int(off[-1])
    pkt_of_cell = np.repeat(np.arange(len(lens_np), dtype=np.int64), cells)
    within = np.arange(C, dtype=np.int64) - off[pkt_of_cell]
    slot_cell_idx = pkt_of_cell * cells_per_slot + within
    return C, slot_cell_idx


def host_io_phase(launcher, pristine, lens, lens_np, args, now_sec,
                  steps, warmup):
    """Host-boundary throughput: packets cross PCIe both ways every step
    (round-1 VERDICT task 1 — no measured number previously included the
    host boundary).  Pipeline per slot: pinned-host packed batch
    --H2D--> unpack to stride slots --uplink kernel--> pack --D2H-->
    pinned host.  H2D, compute, and D2H overlap across in-flight slots
    on three streams, the DMA-conveyor steady state.

    Returns (host_mpps, per_step_s list, pipe_lat_s list)."""
    import torch
    device = launcher.device
    stride = args.stride
    n = lens.numel()
    C, slot_idx_np = build_cell_map(lens_np, stride)
    slot_idx = torch.from_numpy(slot_idx_np).to(device)

    # packed pinned-host input: gather the pristine batch's cells once
    dev_packed_in = torch.index_select(
        pristine.view(-1, 64), 0, slot_idx).contiguous()
    host_in = torch.empty((C, 64), dtype=torch.uint8, pin_memory=True)
    host_in.copy_(dev_packed_in)
    del dev_packed_in

    nbuf = 3
    din = [torch.empty((C, 64), dtype=torch.uint8, device=device)
           for _ in range(nbuf)]
    dout = [torch.empty((C, 64), dtype=torch.uint8, device=device)
            for _ in range(nbuf)]
    works = [torch.empty((n, stride), dtype=torch.uint8, device=device)
             for _ in range(nbuf)]
    hout = [torch.empty((C, 64), dtype=torch.uint8, pin_memory=True)
            for _ in range(nbuf)]
    clss = [torch.empty(n, dtype=torch.uint8, device=device)
            for _ in range(nbuf)]
    orders = [torch.zeros(n, dtype=torch.int32, device=device)
              for _ in range(nbuf)]

    h2d_stream = torch.cuda.Stream(device=device)
    d2h_stream = torch.cuda.Stream(device=device)
    ev_h2d = [torch.cuda.Event() for _ in range(nbuf)]
    ev_comp = [torch.cuda.Event() for _ in range(nbuf)]
    ev_d2h = [torch.cuda.Event() for _ in range(nbuf)]
    for ev in ev_d2h:
        ev.record()

    base_ns = now_sec * 10**9

    def step(k):
        b = k % nbuf
        with torch.cuda.stream(h2d_stream):
            h2d_stream.wait_event(ev_d2h[b])       # slot free again
            din[b].copy_(host_in, non_blocking=True)   # RX DMA (PCIe H2D)
            ev_h2d[b].record(h2d_stream)
        cur = torch.cuda.current_stream(device)
        cur.wait_event(ev_h2d[b])
        works[b].view(-1, 64).index_copy_(0, slot_idx, din[b])  # ring->slots
        launcher.ext.pkt_class(works[b], lens, clss[b])
        orders[b].copy_(torch.argsort(clss[b], stable=True).to(torch.int32))
        launcher.uplink(works[b], lens, now_ns=base_ns + k * 10**6,
                        now_sec=now_sec, sort_by_type=True, order=orders[b])
        torch.index_select(works[b].view(-1, 64), 0, slot_idx,
                           out=dout[b])            # slots->TX ring
        ev_comp[b].record(cur)
        with torch.cuda.stream(d2h_stream):
            d2h_stream.wait_event(ev_comp[b])
            hout[b].copy_(dout[b], non_blocking=True)  # TX DMA (PCIe D2H)
            ev_d2h[b].record(d2h_stream)

    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    # per-batch completion stamps via timing events on the D2H stream
    # (host syncs inside the loop would serialize the conveyor)
    t_ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    with torch.cuda.stream(d2h_stream):
        t_ev[0].record(d2h_stream)
    for k in range(steps):
        step(warmup + k)
        with torch.cuda.stream(d2h_stream):
            t_ev[k + 1].record(d2h_stream)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_step = [t_ev[k].elapsed_time(t_ev[k + 1]) * 1e-3
                for k in range(steps)]
    host_mpps = n * steps / elapsed / 1e6

    # single-batch pipe latency: host write visible -> TX bytes on host
    pipe_lat = []
    for _ in range(16):
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(0)
        ev_d2h[0].synchronize()
        pipe_lat.append(time.perf_counter() - t)
    return host_mpps, per_step, pipe_lat


def service_latency(launcher, args, now_sec, reps=128, batch=256,
                    flood_steps=0, flood_fn=None,
                    paced_period_s: float = 0.0):
    """DHCP OFFER latency through the persistent service kernel
    (host write -> doorbell -> resident waves -> reply visible on
    host).  flood_steps>0 enqueues that many 1M-packet uplink launches
    first, so the service is measured UNDER a SATURATING data flood —
    the case where the launched path degraded to p99 453us in r1.
    paced_period_s>0 instead paces one flood batch per period (a
    realistic <100% utilization operating point: between batches the
    service CUs run uncontended)."""
    import torch
    from bng_amd.dataplane.launcher import DhcpService
    lat_np, lens_np = gen_batch(batch, args.subs, 1.0, args.stride,
                                seed=881)
    svc = DhcpService(launcher, n_slots=max(256, batch),
                      stride=args.stride, idle_exit_k=400_000)
    try:
        svc.serve(lat_np, lens_np, now_sec)          # warm
        if flood_steps and flood_fn is not None:
            for _ in range(flood_steps):
                flood_fn()
        lats = []
        last_flood = time.perf_counter()
        for _ in range(reps):
            if paced_period_s and flood_fn is not None and \
                    time.perf_counter() - last_flood >= paced_period_s:
                flood_fn()
                last_flood = time.perf_counter()
            t = time.perf_counter()
            v, ol, _rep = svc.serve(lat_np, lens_np, now_sec)
            lats.append((time.perf_counter() - t) * 1e6)
        n_tx = int((v == abi.TX).sum())
        assert n_tx == batch, f"service answered {n_tx}/{batch}"
        # stream-scoped sync: a device-wide synchronize() would block
        # on the resident service kernel
        torch.cuda.current_stream().synchronize()
        lats.sort()
        return lats[len(lats) // 2], lats[int(len(lats) * 0.99)]
    finally:
        svc.stop()


def host_io_dhcp_latency(launcher, args, now_sec, reps=64):
    """Arrival->TX DHCP OFFER latency THROUGH the host boundary: pinned
    request batch -> H2D -> dhcp_fastpath -> D2H replies -> host
    visible.  The reference's <100us P99 target is judged on this
    number plus batching wait (reported separately)."""
    import torch
    device = launcher.device
    lat_np, lat_lens_np = gen_batch(args.lat_batch, args.subs, 1.0,
                                    args.stride, seed=778)
    host_req = torch.from_numpy(lat_np).pin_memory()
    dev = torch.empty((args.lat_batch, args.stride), dtype=torch.uint8,
                      device=device)
    ll = torch.from_numpy(lat_lens_np.view(np.int16)).to(device)
    host_rep = torch.empty(host_req.shape, dtype=torch.uint8,
                           pin_memory=True)
    lats = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        dev.copy_(host_req, non_blocking=True)
        launcher.dhcp_fastpath(dev, ll, now_sec=now_sec)
        host_rep.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
        lats.append((time.perf_counter() - t) * 1e6)
    lats.sort()
    return lats[len(lats) // 2], lats[int(len(lats) * 0.99)]


DUMP_PACKET_ROWS = 8192


def dump_outputs(out_dir, last, rank, world):
    """Write what the last timed step returned to its caller as
    <out_dir>/<name>.npy (float32; rank-suffixed when world>1):
    `verdict` and `out_len` for every packet of the batch, and
    `packets`, a fixed seeded sample of DUMP_PACKET_ROWS full stride-wide
    rows of the in-place rewritten batch (`packet_rows` names them) —
    the whole 1M x 512 B batch would be 2 GB as float32, the sample
    keeps a dump near 25 MB.  Inputs, tables and the sample are all
    seeded, so two runs with the same arguments are comparable file by
    file."""
    import torch
    d, v, ol = last
    os.makedirs(out_dir, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    m = v.numel()
    rows = np.sort(np.random.default_rng(0xD0C5).choice(
        m, size=min(m, DUMP_PACKET_ROWS), replace=False))
    rows_dev = torch.from_numpy(rows).to(d.device)
    outs = {
        "verdict": v.cpu().numpy(),
        "out_len": ol.cpu().numpy(),
        "packet_rows": rows.astype(np.float64),
        "packets": d[:m].index_select(0, rows_dev).cpu().numpy(),
    }
    for name, arr in outs.items():
        if arr.dtype != np.float64:
            arr = arr.astype(np.float32)
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1048576,
                    help="packets injected per GPU per step")
    ap.add_argument("--subs", type=int, default=1_000_000)
    ap.add_argument("--dhcp-frac", type=float, default=0.1)
    ap.add_argument("--stride", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the secondary "
                         "phases (launched-batch DHCP latency, downlink "
                         "return path, persistent-service latency, "
                         "host-boundary conveyor); a plain run measures "
                         "the headline only and reports them as null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed "
                         "step returned (verdict, out_len, a fixed seeded "
                         "sample of the rewritten packet rows) as "
                         "DIR/<name>.npy")
    ap.add_argument("--lat-batch", type=int, default=2048)
    ap.add_argument("--lat-reps", type=int, default=64)
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-host-io", action="store_true",
                    help="skip the host-boundary (PCIe-crossing) phase")
    ap.add_argument("--host-io-steps", type=int, default=12)
    ap.add_argument("--host-io-warmup", type=int, default=4)
    ap.add_argument("--svc-cus", type=int, default=0,
                    help="EXPERIMENTAL: reserve N CUs for the service "
                         "via CU-masked streams — currently hangs "
                         "kernel completion on ROCm 7.0/gfx950 "
                         "(R02_EVIDENCE.md); leave 0")
    ap.add_argument("--no-sort", action="store_true",
                    help="disable on-device type-sort (wave-divergence fix)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="disable RX-copy/steer/sort overlap with the "
                         "previous batch's pipeline kernel")
    ap.add_argument("--steer-all", action="store_true",
                    help="world>1: draw data traffic uniformly (every "
                         "packet crosses xGMI) instead of the RSS-steered "
                         "arrival model")
    args = ap.parse_args()

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if distributed:
        import torch.distributed as dist
        # clamp for single-GPU multi-rank rehearsals (RCCL co-located
        # ranks); on a real N-GPU node device_count >= local_rank and
        # this is a no-op
        local_rank = min(local_rank, torch.cuda.device_count() - 1)
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl")
    device = f"cuda:{local_rank}"

    now_sec = 1_700_000_000
    from bng_amd.dataplane.launcher import HipLauncher
    from bng_amd.parallel.sharding import ExchangeBuffers, exchange

    t0 = time.perf_counter()
    # size tables for the subscriber count (load factor <= 0.5)
    base_log2 = max(18, (args.subs - 1).bit_length() + 1)
    launcher = HipLauncher(
        device, sub_log2=base_log2, sess_log2=base_log2 + 1,
        eim_log2=base_log2, subnat_log2=base_log2, qos_log2=base_log2,
        binding_log2=base_log2, svc_cus=args.svc_cus)
    launcher.set_server_config(b"\x02\x00\x00\x00\x00\x01",
                               ip2u32("10.255.255.1"))
    launcher.add_pool(1, ip2u32("10.0.0.0"), 8, ip2u32("10.255.255.1"),
                      ip2u32("8.8.8.8"), ip2u32("1.1.1.1"), 86400)
    launcher.set_antispoof_config(default_mode=abi.AS_DISABLED)
    build_tables(launcher, rank, world, args.subs, now_sec)
    log(rank, f"[bench] tables built in {time.perf_counter() - t0:.1f}s")

    t0 = time.perf_counter()
    data_np, lens_np = gen_batch(args.batch, args.subs, args.dhcp_frac,
                                 args.stride, seed=1234 + rank, rank=rank,
                                 world=world, steer_all=args.steer_all)
    pristine = torch.from_numpy(data_np).to(device)
    lens = torch.from_numpy(lens_np.view(np.int16)).to(device)
    log(rank, f"[bench] batch generated in {time.perf_counter() - t0:.1f}s")

    overlap = not args.no_overlap
    # 4 in-flight batches hide prep-sync slack behind the kernel
    # (same-box A/B: nbuf 2/3/4 -> 1537/1555/1567 Mpps); BNG_NBUF
    # overrides for experiments
    nbuf = (int(os.environ.get("BNG_NBUF", "4")) if overlap else 1)
    if args.dump_outputs and overlap and nbuf < 2:
        # with one buffer the next batch's RX copy lands on the last
        # step's packets before they can be written out
        ap.error("--dump-outputs with overlap needs BNG_NBUF >= 2")
    works = [torch.empty_like(pristine) for _ in range(nbuf)]
    clss = [torch.empty(args.batch, dtype=torch.uint8, device=device)
            for _ in range(nbuf)]
    # persistent cross-stream buffers: the order tensor is produced on
    # the prep stream and consumed on the main stream, so it must NOT be
    # a prep-stream temporary (the caching allocator would recycle it
    # while the main-stream kernel still reads it)
    orders = [torch.zeros(args.batch, dtype=torch.int32, device=device)
              for _ in range(nbuf)]
    # pre-allocated recv-side exchange buffers, one set per in-flight
    # batch (no per-step prep-stream allocations with RCCL in the loop);
    # 2x capacity covers hashring skew + steer-all variance
    exbufs = [ExchangeBuffers(2 * args.batch, args.stride, device, world)
              for _ in range(nbuf)] if distributed else None
    prep_stream = torch.cuda.Stream(device=device) if overlap else None  # noqa: E501
    prep_done = [torch.cuda.Event() for _ in range(nbuf)]
    work_free = [torch.cuda.Event() for _ in range(nbuf)]
    for ev in work_free:
        ev.record()

    batches = [None] * nbuf

    def prep(k):
        """RX copy (+ xGMI steering of DHCP strays when world>1) +
        classify + type-sort for step k — on the prep stream, overlapped
        with step k-1's pipeline kernel (and its collectives)."""
        b = k % nbuf
        with torch.cuda.stream(prep_stream):
            prep_stream.wait_event(work_free[b])
            works[b].copy_(pristine)               # RX-DMA analog
            d, l = works[b], lens
            if distributed:
                owner = launcher.shard_owner(d, l, world)
                d, l = exchange(d, l, owner, bufs=exbufs[b])
            o = None
            if not args.no_sort:
                if d is works[b]:
                    launcher.ext.pkt_class(d, l, clss[b])
                    idx = torch.argsort(clss[b], stable=True)
                    orders[b].copy_(idx.to(torch.int32))
                    o = orders[b]
                else:
                    # exchanged batch: size varies per rank; classify
                    # and sort into this slot's persistent scratch
                    m = l.numel()
                    cls = exbufs[b].cls[:m]
                    launcher.ext.pkt_class(d, l, cls)
                    o = exbufs[b].order[:m]
                    o.copy_(torch.argsort(cls, stable=True)
                            .to(torch.int32))
            batches[b] = (d, l, o)
            prep_done[b].record(prep_stream)

    # what the latest step handed back to its caller: (packets rewritten
    # in place, verdict, out_len) — kept for --dump-outputs
    last = [None]

    def step(now_ns, k=0):
        cur = torch.cuda.current_stream(device)
        if overlap:
            b = k % nbuf
            cur.wait_event(prep_done[b])
            d, l, o = batches[b]
            v, ol = launcher.uplink(d, l, now_ns=now_ns, now_sec=now_sec,
                                    sort_by_type=not args.no_sort, order=o)
            last[0] = (d, v, ol)
            work_free[b].record(cur)
            prep(k + 1)                            # overlap next batch
            return
        works[0].copy_(pristine)                   # RX-DMA analog
        d, l = works[0], lens
        if distributed:
            owner = launcher.shard_owner(d, l, world)
            d, l = exchange(d, l, owner)
        v, ol = launcher.uplink(d, l, now_ns=now_ns, now_sec=now_sec,
                                sort_by_type=not args.no_sort)
        last[0] = (d, v, ol)
    if overlap:
        prep(0)

    base_ns = now_sec * 10**9
    for w in range(args.warmup):
        step(base_ns + w * 10**6, w)
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()

    t_start = time.perf_counter()
    for k in range(args.steps):
        step(base_ns + (args.warmup + k) * 10**6, args.warmup + k)
    torch.cuda.synchronize()
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    elapsed = time.perf_counter() - t_start
    if distributed:
        import torch.distributed as dist
        e = torch.tensor([elapsed], device=device)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())

    total_pkts = world * args.batch * args.steps
    mpps = total_pkts / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last[0], rank, world)

    # everything below is secondary to the headline: --full only
    # p50 DHCP OFFER latency: small all-DHCP batches, submit -> reply ready
    p50_us = p99_us = None
    if args.full and not args.no_latency and rank == 0:
        lat_np, lat_lens_np = gen_batch(args.lat_batch, args.subs, 1.0,
                                        args.stride, seed=777)
        lp = torch.from_numpy(lat_np).to(device)
        lw = torch.empty_like(lp)
        ll = torch.from_numpy(lat_lens_np.view(np.int16)).to(device)
        lats = []
        for r in range(args.lat_reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            lw.copy_(lp)
            launcher.dhcp_fastpath(lw, ll, now_sec=now_sec)
            torch.cuda.synchronize()
            lats.append((time.perf_counter() - t) * 1e6)
        lats.sort()
        p50_us = lats[len(lats) // 2]
        p99_us = lats[int(len(lats) * 0.99)]
        st = launcher.get_stats()
        hits = st["fastpath_hits"]
        log(rank, f"[bench] dhcp stats {st}")
        log(rank, f"[bench] nat stats {launcher.nat_get_stats()}")
        log(rank, f"[bench] p50 {p50_us:.1f}us p99 {p99_us:.1f}us "
                  f"({args.lat_batch}-pkt DHCP batch)")

    # downlink return path: craft internet->subscriber packets against
    # the NAT sessions the uplink loop just established and run the
    # fused DNAT + egress-QoS pipeline (driver-visible counterpart of
    # the uplink headline)
    downlink_mpps = None
    if args.full and rank == 0 and world == 1:
        try:
            recs = launcher.export_nat_sessions()
            if len(recs) >= 1000:
                m = min(len(recs), args.batch)
                sel = recs[:m]
                ret = np.zeros((args.batch, args.stride), dtype=np.uint8)
                rlens = np.full(args.batch, 64, dtype=np.uint16)
                t = np.frombuffer(build_ipv4(
                    "02:00:00:00:00:01", "aa:00:00:00:00:00",
                    ip2u32("93.184.216.34"), ip2u32("203.0.113.1"),
                    proto=17, sport=53, dport=1024,
                    payload=b"\x00" * 22), dtype=np.uint8)
                idxs = np.arange(args.batch) % m
                ret[:, :64] = t
                ret[:, 26:30] = sel["dst_ip"][idxs].astype(">u4") \
                    .view(np.uint8).reshape(-1, 4)
                ret[:, 30:34] = sel["nat_ip"][idxs].astype(">u4") \
                    .view(np.uint8).reshape(-1, 4)
                ret[:, 34:36] = sel["dst_port"][idxs].astype(">u2") \
                    .view(np.uint8).reshape(-1, 2)
                ret[:, 36:38] = sel["nat_port"][idxs].astype(">u2") \
                    .view(np.uint8).reshape(-1, 2)
                dl = torch.from_numpy(ret).to(device)
                dlw = torch.empty_like(dl)
                dll = torch.from_numpy(rlens.view(np.int16)).to(device)
                for k in range(3):
                    dlw.copy_(dl)
                    launcher.downlink(dlw, dll, now_ns=base_ns + k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(10):
                    dlw.copy_(dl)
                    launcher.downlink(dlw, dll,
                                      now_ns=base_ns + 10**6 * k)
                torch.cuda.synchronize()
                downlink_mpps = round(
                    args.batch * 10 / (time.perf_counter() - t0) / 1e6, 1)
                log(rank, f"[bench] downlink {downlink_mpps} Mpps over "
                          f"{len(recs)} live sessions")
        except Exception as e:    # noqa: BLE001 — report, don't fail
            log(rank, f"[bench] downlink phase failed: {e}")

    # persistent-service latency: quiesced and under a saturating data
    # flood (round-1 VERDICT tasks 4/10 — launched-path flood p99 was
    # 453us; the resident waves own their CU so the flood cannot starve
    # them)
    svc_lat = None
    if args.full and not args.no_latency and rank == 0 and world == 1:
        try:
            flood = lambda: step(base_ns, args.warmup + args.steps)  # noqa: E731,E501
            q50, q99 = service_latency(launcher, args, now_sec)
            f50, f99 = service_latency(launcher, args, now_sec,
                                       flood_steps=48, flood_fn=flood)
            torch.cuda.synchronize()
            # ~75% utilization: one 1M-pkt batch per 0.9ms (batch takes
            # ~0.67ms) — the realistic high-load operating point
            l50, l99 = service_latency(launcher, args, now_sec,
                                       reps=256, flood_fn=flood,
                                       paced_period_s=0.0009)
            torch.cuda.synchronize()
            svc_lat = {"svc_p50_us": round(q50, 1),
                       "svc_p99_us": round(q99, 1),
                       "svc_load75_p50_us": round(l50, 1),
                       "svc_load75_p99_us": round(l99, 1),
                       "svc_flood_p50_us": round(f50, 1),
                       "svc_flood_p99_us": round(f99, 1)}
            log(rank, f"[bench] persistent-service latency {svc_lat}")
        except Exception as e:       # noqa: BLE001 — report, don't fail
            svc_lat = {"error": str(e)[:200]}
            log(rank, f"[bench] persistent-service failed: {e}")

    # host-boundary phase: every packet crosses PCIe both ways (the
    # number round 1 lacked: a "host-fed rate" distinct from the GPU
    # pipeline rate).  world==1 only: each GPU has its own PCIe link, so
    # the per-GPU host-fed rate is the scaling unit.
    hostio = None
    if args.full and not args.no_host_io and rank == 0 and world == 1:
        hm, per_step, pipe_lat = host_io_phase(
            launcher, pristine, lens, lens_np, args, now_sec,
            args.host_io_steps, args.host_io_warmup)
        # latency-oriented operating point: 128k-packet batches trade
        # ~10% of the PCIe-bound rate for ~8x lower arrival->TX
        nsmall = min(args.batch, 131072)
        hm_s, per_step_s, pipe_lat_s = host_io_phase(
            launcher, pristine[:nsmall], lens[:nsmall],
            lens_np[:nsmall], args, now_sec,
            args.host_io_steps, args.host_io_warmup)
        hp50, hp99 = host_io_dhcp_latency(launcher, args, now_sec)
        # arrival->TX distribution incl. batching wait: a packet arrives
        # uniformly within its batch accumulation window (one period)
        # and completes at its batch's D2H; latency = wait + residence
        period = float(np.median(per_step))
        res = float(np.median(pipe_lat))
        u = np.random.default_rng(3).uniform(0, period, 20000)
        arr = u + res
        hostio = {
            "host_fed_mpps": round(hm, 1),
            "host_batch_period_us": round(period * 1e6, 1),
            "host_pipe_residence_us_p50": round(
                float(np.percentile(pipe_lat, 50)) * 1e6, 1),
            "host_pipe_residence_us_p99": round(
                float(np.percentile(pipe_lat, 99)) * 1e6, 1),
            "arrival_to_tx_us_p50": round(
                float(np.percentile(arr, 50)) * 1e6, 1),
            "arrival_to_tx_us_p99": round(
                float(np.percentile(arr, 99)) * 1e6, 1),
            "host_dhcp_p50_us": round(hp50, 1),
            "host_dhcp_p99_us": round(hp99, 1),
        }
        period_s = float(np.median(per_step_s))
        res_s = float(np.median(pipe_lat_s))
        arr_s = (np.random.default_rng(4).uniform(0, period_s, 20000)
                 + res_s)
        hostio["small_batch"] = {
            "batch": nsmall,
            "host_fed_mpps": round(hm_s, 1),
            "arrival_to_tx_us_p50": round(
                float(np.percentile(arr_s, 50)) * 1e6, 1),
            "arrival_to_tx_us_p99": round(
                float(np.percentile(arr_s, 99)) * 1e6, 1),
        }
        log(rank, f"[bench] host-io {hostio}")

    if distributed:
        import torch.distributed as dist
        dist.barrier()     # hold all ranks until rank 0's latency phase

    if rank == 0:
        result = {
            "metric": "mpps",
            "value": round(mpps, 3),
            "unit": "Mpps",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(mpps / BASELINE_MPPS, 3),
            "dtype": "uint8",
            "data": "synthetic",
            "config": {
                "model": "bng-uplink-pipeline "
                         "(dhcp_fastpath+antispoof+nat44+qos)",
                "benchmark": "Mpps + p50 DHCP OFFER latency, 64B mix, "
                             "1M-sub table at 1/2/4/8 MI355X",
                "global_batch": world * args.batch,
                "seq_len": args.stride,
                "svc_cus": args.svc_cus,
                "parallelism": f"shard{world}-rss" +
                               ("-steerall" if args.steer_all else
                                "-dhcp-alltoall"),
                "n_subscribers": args.subs,
                "dhcp_frac": args.dhcp_frac,
                "p50_dhcp_offer_us": None if p50_us is None
                else round(p50_us, 1),
                "p99_dhcp_offer_us": None if p99_us is None
                else round(p99_us, 1),
                "baseline_mpps": BASELINE_MPPS,
                "host_io": hostio,
                "downlink_mpps": downlink_mpps,
                "persistent_service": svc_lat,
            },
        }
        print(json.dumps(result), flush=True)

    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
