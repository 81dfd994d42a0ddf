"""Token-bucket and NAT-timeout time arithmetic on the device, exactly.

Both decide from `now_ns` minus a stored stamp whether a subscriber's
packets or flows survive.  Everything here is integer arithmetic and every
comparison is exact.

The bucket (`qos_tb_check`) runs behind four entry points: the stand-alone
QoS kernel on the egress table and on the subscriber contexts, the fused
uplink (ingress policy next to a NAT context) and the fused downlink.  Each
is driven with one packet per bucket per launch, the shape at which the
kernel is deterministic, at n = 1, 64 and 65 buckets, and after every
launch the verdicts, every bucket's `tokens` and `last_update` as read back
from the raw table, and the QoS counters are compared with
`lazy_bucket.LazyBucket`.  The tables have 64 slots; 65 buckets need 128.

The sweeper (`nat_sweep_kernel`) is compared with `GoldenLauncher.sweep_nat`
on identical state, one nanosecond either side of every timeout and with
the clock stepped back behind `last_seen`.
"""
import pytest

pytestmark = pytest.mark.gpu

import test_uplink_snapshots_gpu as snap
from bng_amd.dataplane import abi
from bng_amd.dataplane.launcher import (EIM_TIMEOUT_NS, ICMP_TIMEOUT_NS,
                                        TCP_EST_TIMEOUT_NS,
                                        TCP_TRANSIENT_TIMEOUT_NS,
                                        UDP_TIMEOUT_NS)
from bng_amd.dataplane.packets import build_ipv4, ip2u32
from lazy_bucket import LazyBucket, exact_credit

NOW = snap.NOW_NS
MS = snap.MS
SEC = 10**9
U64 = 1 << 64
PEER = snap.DST
PUB = ip2u32("203.0.113.1")
CORE_MAC = bytes.fromhex("020000000002")
FWD, DROP = abi.FWD, abi.DROP

ENTRIES = ["qos-egress", "qos-ingress", "uplink", "downlink"]
BATCH = [1, 64, 65]


# ================================================================ the rig
class Rig:
    """One device launcher behind one entry point; bucket k belongs to
    subscriber k and is keyed by its address."""

    def __init__(self, entry, n):
        log2 = 6 if n <= 64 else 7
        self.entry = entry
        self.ingress = entry in ("qos-ingress", "uplink")
        self.gpu = snap.hip_launcher(qos_log2=log2, subnat_log2=log2)
        if entry == "uplink":
            for k in range(n):
                self.gpu.add_subscriber_nat(snap.sub_ip(k), PUB,
                                            1024 + 64 * k, 1087 + 64 * k,
                                            subscriber_id=k + 1)

    def set_buckets(self, buckets):
        """Write every field of every bucket, in one upsert."""
        import torch
        gpu = self.gpu
        if self.ingress:
            raw = b"".join(bytes(abi.SubCtx(
                key_ip=snap.sub_ip(k), rate_bps=b.rate_bps, tokens=b.tokens,
                last_update=b.last_update, burst_bytes=b.burst))
                for k, b in enumerate(buckets))
        else:
            raw = b"".join(bytes(abi.QosBucket(
                key_ip=snap.sub_ip(k), valid=1, rate_bps=b.rate_bps,
                tokens=b.tokens, last_update=b.last_update,
                burst_bytes=b.burst)) for k, b in enumerate(buckets))
        rc = torch.full((len(buckets),), -7, dtype=torch.int32,
                        device=gpu.device)
        if self.ingress:
            gpu.ext.subctx_upsert(gpu.subctx, gpu._to_dev(raw),
                                  abi.CTX_SET_QOS, rc)
        else:
            gpu.ext.qos_upsert(gpu.qos_egress, gpu._to_dev(raw), rc)
        assert rc.cpu().tolist() == [0] * len(buckets)

    def frame(self, k, length):
        pay = b"\x00" * (length - 42)
        if self.ingress:
            f = build_ipv4(snap.sub_mac(k), snap.SERVER_MAC, snap.sub_ip(k),
                           PEER, proto=17, sport=20000 + k, dport=53,
                           payload=pay)
        else:
            f = build_ipv4(CORE_MAC, snap.SERVER_MAC, PEER, snap.sub_ip(k),
                           proto=17, sport=53, dport=20000 + k, payload=pay)
        assert len(f) == length
        return f

    def launch(self, frames, now):
        gpu = self.gpu
        d, l = gpu.make_batch(frames)
        if self.entry == "uplink":
            v, _ = gpu.uplink(d, l, now_ns=now, now_sec=snap.NOW_SEC)
        elif self.entry == "downlink":
            v = gpu.downlink(d, l, now_ns=now)
        else:
            v = gpu.qos(d, l, egress=not self.ingress, now_ns=now)
        return v.cpu().tolist()

    def buckets(self):
        """{key_ip: (rate, burst, tokens, last_update)} from the raw table."""
        table, cls = (self.gpu.subctx, abi.SubCtx) if self.ingress else \
            (self.gpu.qos_egress, abi.QosBucket)
        blob = table.cpu().numpy().tobytes()
        out = {}
        for off in range(0, len(blob), 64):
            e = cls.from_buffer_copy(blob, off)
            if e.key_ip:
                out[e.key_ip] = (e.rate_bps, e.burst_bytes, e.tokens,
                                 e.last_update)
        return out


def offer_and_check(rig, buckets, lengths, now, tag=""):
    """One launch at `now`, one packet per bucket; verdicts, table and
    counters against the model.  Returns the model's verdicts."""
    before = rig.gpu.qos_get_stats()
    was = [(b.tokens, b.last_update) for b in buckets]
    got = rig.launch([rig.frame(k, L) for k, L in enumerate(lengths)], now)
    want = [b.offer(now, L) for b, L in zip(buckets, lengths)]
    dev = rig.buckets()
    bad = []
    for k, (b, L) in enumerate(zip(buckets, lengths)):
        g = (got[k],) + dev[snap.sub_ip(k)]
        w = (FWD if want[k] else DROP, b.rate_bps, b.burst, b.tokens,
             b.last_update)
        if g != w:
            bad.append(f"{tag} bucket {k}: rate {b.rate_bps} burst {b.burst} "
                       f"(tokens, last_update) {was[k]} now {now} len {L}: "
                       f"(verdict, rate, burst, tokens, last_update) "
                       f"{g} != {w}")
    assert not bad, "\n".join(bad[:12])
    after = rig.gpu.qos_get_stats()
    yes = [L for w, L in zip(want, lengths) if w]
    no = [L for w, L in zip(want, lengths) if not w]
    assert {k: after[k] - before[k] for k in after} == {
        "packets_passed": len(yes), "packets_dropped": len(no),
        "bytes_passed": sum(yes), "bytes_dropped": sum(no)}, tag
    return want


cases = pytest.mark.parametrize(
    "entry,n", [(e, n) for e in ENTRIES for n in BATCH],
    ids=[f"{e}-n{n}" for e in ENTRIES for n in BATCH])


# ======================================================= rate x idle grid
RATES = [64_000, 10**8, 10**9, 10**10, 10**11]
IDLES = [0, 1, 999_999_999, SEC, 14_757_395_259, 20 * SEC, 100 * SEC - 1,
         100 * SEC + 1, 101 * SEC, 3600 * SEC]
GRID = [(rate, idle, 0xFFFFFFFF if wide else rate // 8 // 100)
        for rate in RATES for idle in IDLES for wide in (False, True)]
# past the issue's grid, operands where narrower schemes wrap: the
# sub-second remainder times rate/8 above 2^64 (>= 147 Gbps), a product
# whose high word is just below and just above 1e9, and a stamp of zero
GRID += [(2 * 10**11, 999_999_999, 0xFFFFFFFF),
         (2 * 10**11, 3600 * SEC + 999_999_999, 0xFFFFFFFF),
         (U64 - 1, 7 * SEC, 0xFFFFFFFF),
         (U64 - 1, 10 * SEC, 1500),
         (U64 - 1, NOW, 0xFFFFFFFF),
         (64_000, NOW, 0xFFFFFFFF)]


def grid_len(c):
    return 64 if c % 3 == 0 else 64 + (c * 37) % 400


@cases
def test_rate_idle_grid_from_a_drained_bucket(entry, n):
    """Every (rate, idle, burst) of the grid as a drained bucket stamped
    `idle` before the launch, n at a time.  Holds the three cases a 64-bit
    refill gets wrong: 10 Gbps after 14 757 395 259 ns (the product wraps
    to a credit of 0), 64 kbps after 101 s under a wide burst (808 000 B,
    not the burst), and idle 0 (no refill, no stamp moved)."""
    rig = Rig(entry, n)
    seen = []
    for start in range(0, len(GRID), n):
        idx = [(start + j) % len(GRID) for j in range(n)]
        buckets = [LazyBucket(GRID[c][0], GRID[c][2], 0, NOW - GRID[c][1])
                   for c in idx]
        rig.set_buckets(buckets)
        seen += offer_and_check(rig, buckets, [grid_len(c) for c in idx],
                                NOW, f"grid {idx[0]}..")
    assert True in seen and False in seen


# ======================================================= greedy trajectory
TRAJ_RATES = [64_000, 10**6, 10**7, 10**8, 10**9, 10**10]
TRAJ_STEPS = [1_000, 30_000, 1_000_000, 7_000, 250_000, 3]
TRAJ_LAUNCHES = 256


@cases
def test_greedy_trajectory_matches_the_model(entry, n):
    """256 launches, one packet per bucket each, steps from 3 ns to 3 ms:
    at the slow rates most refills earn nothing or a fraction of a packet
    and still move the stamp, while the buckets that start with tokens
    pass packets without touching it: the stretch where the eager golden
    bucket and the lazy device bucket part.  Verdicts and state are
    compared after every launch, so sum(passed) and the final state are
    the model's."""
    rig = Rig(entry, n)
    lengths = [100 + 3 * (k % 50) for k in range(n)]
    buckets = [LazyBucket(TRAJ_RATES[k % 6], 4 * lengths[k],
                          (k * 131) % (4 * lengths[k] + 1), NOW)
               for k in range(n)]
    rig.set_buckets(buckets)
    now, zero, part, passed = NOW, 0, 0, 0
    for i in range(TRAJ_LAUNCHES):
        now += TRAJ_STEPS[i % 6] * (1 + i % 3)
        for b, L in zip(buckets, lengths):
            if b.tokens < L:                     # this packet will refill
                c = exact_credit(now - b.last_update, b.rate_bps)
                zero += c == 0
                part += 0 < c < L
        passed += sum(offer_and_check(rig, buckets, lengths, now,
                                      f"launch {i}"))
    assert zero > 0 and part > 0
    assert 0 < passed < n * TRAJ_LAUNCHES


# ========================================================== backward clock
@cases
def test_clock_stepped_back_behind_the_stamp(entry, n):
    """now = last_update - 1 and now = last_update - 10 s, on a drained and
    on a full bucket: no credit, the stamp stays, the verdict is the plain
    consume's.  An unsigned difference would credit the whole burst.  Once
    the clock has passed the stamp again, credit counts from the stamp."""
    rig = Rig(entry, n)
    burst, L = 10_000, 200
    for shift in range(4 if n < 4 else 1):
        kinds = [((k + shift) % 2, ((k + shift) // 2) % 2) for k in range(n)]
        back = [(1, 10 * SEC)[far] for far, _ in kinds]
        buckets = [LazyBucket(RATES[k % 5], burst, burst if full else 0,
                              NOW + back[k])
                   for k, (_, full) in enumerate(kinds)]
        rig.set_buckets(buckets)
        want = offer_and_check(rig, buckets, [L] * n, NOW, "back")
        for k, (b, (_, full)) in enumerate(zip(buckets, kinds)):
            assert want[k] == bool(full)
            assert b.last_update == NOW + back[k]
            assert b.tokens == (burst - L if full else 0)
        offer_and_check(rig, buckets, [L] * n, NOW + 10 * SEC + MS, "ahead")
        assert all(b.last_update == NOW + 10 * SEC + MS
                   for b, (_, full) in zip(buckets, kinds) if not full)


# ======================================================== contended refill
@pytest.mark.parametrize("credit_pkts", [3, 300, 0])
@pytest.mark.parametrize("entry", ENTRIES)
def test_contended_refill_mints_nothing(entry, credit_pkts, capsys):
    """256 equal packets in one launch to one drained bucket whose refill is
    worth 3 packets, 300 packets under a burst of 10, or nothing.  Which
    packets pass is up to thread order; what must hold is conservation:
    nothing minted, no debt left, and the design bound of one burst plus
    the 255 debits that can be in flight while the refill caps.

    The refill caps `cur + add` on a `cur` that other packets' failed
    consumes have debited for a moment, so their restores could lift
    `tokens` above `burst` until the next refill.  From a drained bucket
    the credit itself is clamped to the burst, which leaves no room for
    that here.  Observed on an MI355X: tokens_after stayed at or below
    burst in all twelve cases (overshoot 0)."""
    L, rate, burst = 125, 10**9, 10 * 125       # 125 bytes per microsecond
    idle = credit_pkts * 1000 if credit_pkts else 1
    add = exact_credit(idle, rate)
    assert add == credit_pkts * L
    rig = Rig(entry, 1)
    if entry == "uplink":                       # the flow's session exists
        assert rig.launch([rig.frame(0, L)], NOW - SEC) == [FWD]
    rig.set_buckets([LazyBucket(rate, burst, 0, NOW)])
    key, now = snap.sub_ip(0), NOW + idle
    before = rig.gpu.qos_get_stats()

    got = rig.launch([rig.frame(0, L)] * 256, now)
    _, _, tokens, last = rig.buckets()[key]
    passed = got.count(FWD)
    with capsys.disabled():
        print(f"\n[contended {entry} credit {credit_pkts} pkts] passed "
              f"{passed}/256, tokens_after {tokens}, burst {burst}, "
              f"overshoot {max(0, tokens - burst)}")
    assert passed + got.count(DROP) == 256 and last == now
    assert tokens >= 0
    assert passed * L + tokens <= 0 + add
    assert passed * L + tokens <= min(burst, 0 + add) + 255 * L

    got2 = rig.launch([rig.frame(0, L)] * 256, now)
    _, _, tokens2, last2 = rig.buckets()[key]
    passed2 = got2.count(FWD)
    assert last2 == now and 0 <= tokens2 <= burst
    assert passed2 * L + tokens2 == tokens       # no refill at the same now
    after = rig.gpu.qos_get_stats()
    assert {k: after[k] - before[k] for k in after} == {
        "packets_passed": passed + passed2,
        "packets_dropped": 512 - passed - passed2,
        "bytes_passed": (passed + passed2) * L,
        "bytes_dropped": (512 - passed - passed2) * L}


# ================================================================= sweeper
KINDS = ["udp", "icmp", "tcp-new", "tcp-est", "tcp-closing"]
PROTO = {"udp": 17, "icmp": 1, "tcp-new": 6, "tcp-est": 6, "tcp-closing": 6}
STATE = {"udp": abi.NAT_NEW, "icmp": abi.NAT_NEW, "tcp-new": abi.NAT_NEW,
         "tcp-est": abi.NAT_ESTABLISHED, "tcp-closing": abi.NAT_CLOSING}
TIMEOUT = {"udp": UDP_TIMEOUT_NS, "icmp": ICMP_TIMEOUT_NS,
           "tcp-new": TCP_TRANSIENT_TIMEOUT_NS,
           "tcp-est": TCP_EST_TIMEOUT_NS,
           "tcp-closing": TCP_TRANSIENT_TIMEOUT_NS}
SYN, ACK, SYN_ACK, FIN_ACK = 0x02, 0x10, 0x12, 0x11


def nat_pair(n_subs):
    gpu, cpu = snap.make_pair(sess_log2=6, eim_log2=6, subnat_log2=6)
    for l in (gpu, cpu):
        for k in range(n_subs):
            l.add_subscriber_nat(snap.sub_ip(k), PUB, 1024 + 64 * k,
                                 1087 + 64 * k, subscriber_id=k + 1)
    return gpu, cpu


def flow_key(k, kind, dst=PEER):
    if PROTO[kind] == 1:
        return (snap.sub_ip(k), dst, 700 + k, 0, 1)
    return (snap.sub_ip(k), dst, 20000 + k, 443, PROTO[kind])


def out_frame(k, kind, pad=0, dst=PEER):
    return build_ipv4(snap.sub_mac(k), snap.SERVER_MAC, snap.sub_ip(k), dst,
                      proto=PROTO[kind], sport=20000 + k, dport=443,
                      icmp_id=700 + k, tcp_flags=SYN, payload=b"\x00" * pad)


def back_frame(wire, kind, flags=ACK, pad=0):
    """The peer's answer to a translated outbound frame."""
    nat_ip = int.from_bytes(wire[26:30], "big")
    port = int.from_bytes(wire[38:40] if PROTO[kind] == 1 else wire[34:36],
                          "big")
    return build_ipv4(CORE_MAC, snap.SERVER_MAC, PEER, nat_ip,
                      proto=PROTO[kind], sport=443, dport=port, icmp_id=port,
                      tcp_flags=flags, payload=b"\x00" * pad)


def drive(pair, frames, egress, now):
    """The frames through nat44 on both; verdicts and bytes must agree.
    Returns the frames as they leave."""
    gpu, cpu = pair
    d, l = gpu.make_batch(frames)
    v = gpu.nat44(d, l, egress=egress, now_ns=now).cpu().tolist()
    rows = d.cpu().numpy()
    res = cpu.process_nat44(frames, egress=egress, now_ns=now)
    for i, (f, (wv, wb)) in enumerate(zip(frames, res)):
        assert v[i] == wv, f"frame {i}: verdict {v[i]} != {wv}"
        assert rows[i, :len(f)].tobytes() == wb, f"frame {i}: bytes differ"
    return [wb for _, wb in res]


def eim_table(gpu):
    blob = gpu.eim.cpu().numpy().tobytes()
    out = {}
    for off in range(0, len(blob), 48):
        e = abi.EimEntry.from_buffer_copy(blob, off)
        if e.sig not in (0, U64 - 1):
            assert e.ready == 1
            out[(e.internal_ip, e.internal_port, e.protocol)] = (
                e.external_ip, e.external_port, e.created, e.last_used,
                e.ref_count)
    return out


def sessions_active(gpu):
    blob = gpu.subctx.cpu().numpy().tobytes()
    ctx = [abi.SubCtx.from_buffer_copy(blob, off)
           for off in range(0, len(blob), 64)]
    return {e.key_ip: e.sessions_active for e in ctx if e.key_ip}


def same_nat_state(pair, tag=""):
    gpu, cpu = pair
    assert snap.session_table(gpu, inbound=True) == \
        snap.golden_session_table(cpu, inbound=True), tag
    assert eim_table(gpu) == {
        k: (e.external_ip, e.external_port, e.created, e.last_used,
            e.ref_count) for k, e in cpu.dp.eim.items()}, tag
    assert gpu.nat_get_stats() == cpu.nat_get_stats(), tag
    assert sessions_active(gpu) == {
        ip: b.sessions_active for ip, b in cpu.dp.subnat.items()}, tag


def sweep(pair, now):
    for l in pair:
        l.sweep_nat(now_ns=now)


def one_of_each(pair, t0):
    """Subscriber k holds one session of KINDS[k].  Returns the translated
    outbound frames and each session's last_seen."""
    wire = drive(pair, [out_frame(k, kind) for k, kind in enumerate(KINDS)],
                 True, t0)
    drive(pair, [back_frame(wire[3], "tcp-est", SYN_ACK),
                 back_frame(wire[4], "tcp-closing", SYN_ACK)], False, t0 + MS)
    drive(pair, [back_frame(wire[4], "tcp-closing", FIN_ACK)], False,
          t0 + 2 * MS)
    seen = {"udp": t0, "icmp": t0, "tcp-new": t0, "tcp-est": t0 + MS,
            "tcp-closing": t0 + 2 * MS}
    for k, kind in enumerate(KINDS):
        s = pair[1].dp.nat_sessions[flow_key(k, kind)]
        assert (s.state, s.last_seen) == (STATE[kind], seen[kind])
    same_nat_state(pair, "setup")
    return wire, seen


@pytest.mark.parametrize("when", ["one-short", "on-time", "clock-back"])
@pytest.mark.parametrize("kind", KINDS)
def test_sweep_on_each_timeout_boundary(kind, when):
    """last_seen + timeout - 1 keeps the session, last_seen + timeout
    expires it, last_seen - 1 (the clock stepped back) keeps it; the other
    four sessions and the EIM entries go as the golden sweep says.  Then
    the peer answers: translated if the session was kept, left with the
    public address if not."""
    pair = nat_pair(len(KINDS))
    wire, seen = one_of_each(pair, NOW)
    k = KINDS.index(kind)
    at = seen[kind] + {"one-short": TIMEOUT[kind] - 1,
                       "on-time": TIMEOUT[kind], "clock-back": -1}[when]
    sweep(pair, at)
    kept = when != "on-time"
    assert (flow_key(k, kind) in pair[1].dp.nat_sessions) == kept
    if when == "clock-back":
        assert len(pair[1].dp.nat_sessions) == len(KINDS)
        assert len(pair[1].dp.eim) == len(KINDS)
        assert pair[1].nat_get_stats()["sessions_expired"] == 0
    same_nat_state(pair, "after the sweep")
    [answer] = drive(pair, [back_frame(wire[k], kind)], False, at)
    dst = int.from_bytes(answer[30:34], "big")
    assert dst == (snap.sub_ip(k) if kept else PUB)
    same_nat_state(pair, "after the answer")


@pytest.mark.parametrize("when", ["one-short", "on-time", "clock-back"])
def test_sweep_on_the_eim_boundary(when):
    """The same three times for an endpoint-independent mapping.  A second
    flow from the same source port then reuses the mapping if it was kept
    and allocates a new one if not."""
    pair = nat_pair(1)
    drive(pair, [out_frame(0, "udp")], True, NOW)
    at = NOW + {"one-short": EIM_TIMEOUT_NS - 1, "on-time": EIM_TIMEOUT_NS,
                "clock-back": -1}[when]
    sweep(pair, at)
    kept = when != "on-time"
    assert ((snap.sub_ip(0), 20000, 17) in pair[1].dp.eim) == kept
    same_nat_state(pair, "after the sweep")
    drive(pair, [out_frame(0, "udp", dst=PEER + 1)], True, at + MS)
    st = pair[1].nat_get_stats()
    assert (st["eim_hits"], st["eim_misses"]) == ((1, 1) if kept else (0, 2))
    same_nat_state(pair, "after the second flow")


def test_sweep_splits_a_mixed_table_of_40_sessions():
    """Eight subscribers per kind in a 64-slot table, created in three
    generations 100 s apart, swept once at +260 s: every UDP, ICMP, new and
    closing kind loses some sessions and keeps others (one ICMP session is
    1 ns short of its timeout), every established one stays."""
    pair = nat_pair(40)
    kind_of = [KINDS[k % 5] for k in range(40)]
    starts = [NOW, NOW + 100 * SEC + 1, NOW + 200 * SEC + 1]
    for g, t0 in enumerate(starts):
        ks = [k for k in range(40) if (k // 5) % 3 == g]
        wire = dict(zip(ks, drive(
            pair, [out_frame(k, kind_of[k], pad=k % 7) for k in ks], True,
            t0)))
        drive(pair, [back_frame(wire[k], kind_of[k], SYN_ACK) for k in ks
                     if kind_of[k] in ("tcp-est", "tcp-closing")], False,
              t0 + MS)
        drive(pair, [back_frame(wire[k], kind_of[k], FIN_ACK) for k in ks
                     if kind_of[k] == "tcp-closing"], False, t0 + 2 * MS)
    same_nat_state(pair, "setup")
    assert len(pair[1].dp.nat_sessions) == 40
    sweep(pair, NOW + 260 * SEC)
    left = {kind: sum(flow_key(k, kind_of[k]) in pair[1].dp.nat_sessions
                      for k in range(40) if kind_of[k] == kind)
            for kind in KINDS}
    assert left["tcp-est"] == 8
    assert all(0 < left[kind] < 8 for kind in KINDS if kind != "tcp-est")
    same_nat_state(pair, "after the sweep")


def raw_sessions(gpu):
    """{tuple: NatSession} of the live entries, nothing folded."""
    blob = gpu.sessions.cpu().numpy().tobytes()
    out = {}
    for off in range(0, len(blob), 128):
        e = abi.NatSession.from_buffer_copy(blob, off)
        if e.sig not in (0, U64 - 1):
            out[(e.key.src_ip, e.key.dst_ip, e.key.src_port, e.key.dst_port,
                 e.key.protocol)] = e
    return out


def test_sweep_folds_the_packed_counters_of_both_directions():
    """Three launches out and two back with varied lengths leave the hot
    path's packed {bytes:40, pkts:24} words non-zero in both directions;
    a sweep that expires nothing folds them into the 64-bit counters,
    which then equal the golden's, and zeroes the words."""
    pair = nat_pair(6)
    kind_of = [("udp", "icmp", "tcp-est")[k % 3] for k in range(6)]
    for i in range(3):
        wire = drive(pair, [out_frame(k, kind_of[k], pad=(13 * i + 7 * k) % 200)
                            for k in range(6)], True, NOW + i * MS)
    for i in range(2):
        drive(pair, [back_frame(wire[k], kind_of[k], SYN_ACK if i == 0 else
                                ACK, pad=(31 * i + 11 * k) % 300)
                     for k in range(6)], False, NOW + (3 + i) * MS)
    raw = raw_sessions(pair[0])
    assert len(raw) == 6
    assert all(e._pad2[0] and e._pad2[1] for e in raw.values())
    same_nat_state(pair, "before the sweep")       # folds the words itself
    sweep(pair, NOW + 5 * MS)
    raw = raw_sessions(pair[0])
    assert len(raw) == 6 and pair[1].nat_get_stats()["sessions_expired"] == 0
    for key, e in raw.items():
        s = pair[1].dp.nat_sessions[key]
        assert (e.packets_out, e.packets_in, e.bytes_out, e.bytes_in) == \
            (s.packets_out, s.packets_in, s.bytes_out, s.bytes_in) and \
            s.packets_out == 3 and s.packets_in == 2, key
        assert (e._pad2[0], e._pad2[1]) == (0, 0), key
    same_nat_state(pair, "after the sweep")
