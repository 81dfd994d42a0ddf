"""NAT44 port rotor under bursts of ONE subscriber.

Every other NAT test gives each flow a subscriber of its own, so
`nat_alloc_port` never runs with two lanes on one `bng_subctx` at once.  A
subscriber opening a web page is exactly that load.  Here one subscriber
sends a batch of new flows to ONE destination, on a port block the burst
crosses the end of, and the device is compared with `GoldenLauncher`, which
is sequential.

Which flow gets which port depends on lane order, so only order-independent
quantities are compared: the sorted ports, the counters, the block's rotor
and session counts, the exported sessions without their port, and, per
frame, `wire_oracle` (checksums summed from scratch, the datagram rebuilt
the sender's way with the port that frame got).  Step C sends one reply per
translated frame back through DNAT: two flows sharing a public tuple are a
reply delivered to the wrong inner port, which is what the customer sees.

Inputs that keep the port SET deterministic: source ports and ICMP ids are
40000 + i (subject) and 60000 + k (the other subscribers), outside every
block under test, so the in-block EIM-collision heuristic, keyed by
internal port, never fires; every other subscriber carries one flow.

Shapes: 16-port blocks at [2048, 2063] and at the top of the range,
[65520, 65535], and the 1024-port block [64512, 65535] that the NAT
manager hands its 63rd subscriber.  Batches of 16 (one wave, the burst
alone), 64, 65 and 256 + 37 with other subscribers' single flows in
between, the last one forced into a single block (grid cap 1: two
grid-stride iterations, ragged last wave); the wide block with 1024 + 37
frames over five blocks and in one.  Through `nat44()` and through
`uplink()`, plain and with an `order` tensor.

`test_golden_handles_every_scenario` is the CPU half: the same frames
through the golden model alone, with the invariants of steps B, D and E
asserted on ITS output, so a GPU failure cannot be an input the reference
does not handle either.
"""
import random
from collections import Counter

import numpy as np
import pytest

import wire_oracle as wo
from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import DROP, FWD

gpu = pytest.mark.gpu

NOW_SEC = 1_700_000_000
NOW_NS = NOW_SEC * 10**9
MS = 10**6
SENTINEL = 0xA5
SERVER_IP = 0x0AFFFF01                   # 10.255.255.1

LOW16, TOP16, WIDE = (2048, 2063), (65520, 65535), (64512, 65535)
DEST_A = (0xC6336464, 443)               # 198.51.100.100
DEST_B = (wo.DST_IP, 53)
SUBJECT_ID, OTHER_ID = 77, 5
IP_OPTIONS = b"\x01\x01\x01\x00"         # NOP NOP NOP EOL: ihl 6
PRE = 10                                 # flows of step A


# ------------------------------------------------------------- subscribers
def subject(block, k=0):
    return wo.Sub(0x0A640001 + k, (0xAABB00000000 + k).to_bytes(6, "big"),
                  wo.PUBLIC_DEFAULT + k, block[0], block[1])


def other_sub(k):
    """Subscriber k of the crowd: a 512-port block of its own below the
    blocks under test."""
    return wo.Sub(0x0A650001 + k, (0xAACC00000000 + k).to_bytes(6, "big"),
                  wo.PUBLIC_DEFAULT + 16 + k // 100,
                  1024 + (k % 100) * 512, 1024 + (k % 100) * 512 + 511)


# ------------------------------------------------------------------ frames
def payload(i):
    return bytes((i * 7 + j) & 0xFF for j in range(12 + i % 5))


def flow(sub, i, dest, options=b"", proto=None, sport=None):
    """New flow number i of a subscriber: protocols in turn, source port
    and ICMP id 40000 + i.  Every frame is 54 bytes or more, so the
    ihl-5 ones take the register-window parse on an aligned row."""
    proto = wo.PROTOS[i % 3] if proto is None else proto
    sport = 40000 + i if sport is None else sport
    return wo.Entry("subject", wo.build_frame(
        proto, sub.private_ip, dest[0], src_mac=sub.mac, sport=sport,
        dport=dest[1], icmp_id=sport, payload=payload(i), options=options,
        ident=i & 0xFFFF), sub, wo.SCRATCH)


def other_flow(k, dest=DEST_B):
    sub = other_sub(k)
    return wo.Entry("other", wo.build_frame(
        wo.UDP, sub.private_ip, dest[0], src_mac=sub.mac, sport=60000 + k,
        dport=dest[1], payload=payload(k), ident=k), sub, wo.SCRATCH)


def burst(sub, first, m, dest):
    """m new flows of one subscriber to one destination; the first three
    (TCP, UDP, ICMP) carry IP options and take the byte-wise parse."""
    assert first % 3 == 0
    return [flow(sub, first + j, dest, IP_OPTIONS if j < 3 else b"")
            for j in range(m)]


def interleave(mine, n_total):
    """The burst spread evenly over a batch of n_total frames, first and
    last row included; other subscribers' single flows fill the rest."""
    m = len(mine)
    assert n_total >= m > 1
    at = {j * (n_total - 1) // (m - 1): e for j, e in enumerate(mine)}
    assert len(at) == m
    out, k = [], 0
    for row in range(n_total):
        if row in at:
            out.append(at[row])
        else:
            out.append(other_flow(k))
            k += 1
    return out


# --------------------------------------------------------------- launchers
def configure(l, subs, flags):
    l.set_server_config(wo.GW_MAC, SERVER_IP)
    l.add_pool(1, 0x0A010000, 16, 0x0A01FFFE, 0x08080808, 0x01010101, 3600)
    # antispoof lets everything through, and nobody has a QoS policy
    l.set_antispoof_config(default_mode=abi.AS_DISABLED, log_violations=True)
    l.set_nat_config(flags=flags)
    for s, sid in subs:
        l.add_subscriber_nat(s.private_ip, s.public_ip, s.port_start,
                             s.port_end, subscriber_id=sid)
    return l


def golden_launcher(subs, flags=abi.NAT_FLAG_EIM):
    from bng_amd.dataplane.launcher import GoldenLauncher
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    return configure(cpu, subs, flags)


def make_pair(subs, flags=abi.NAT_FLAG_EIM, log2=10):
    """Tables of 2^log2 entries: 10 holds every 16-port scenario, the
    1024-flow bursts take 12."""
    from bng_amd.dataplane.launcher import HipLauncher
    dev = HipLauncher(sub_log2=6, sess_log2=log2, eim_log2=log2,
                      subnat_log2=10, qos_log2=6, binding_log2=6, n_pools=4)
    return configure(dev, subs, flags), golden_launcher(subs, flags)


def with_others(subs, n):
    return [(s, SUBJECT_ID) for s in subs] + \
        [(other_sub(k), OTHER_ID) for k in range(n)]


def set_rotor(dev, cpu, sub, sid, next_port):
    """Put a block's rotor somewhere else than its start, on both."""
    import torch
    e = abi.SubCtx(key_ip=sub.private_ip, subscriber_id=sid,
                   public_ip=sub.public_ip, port_start=sub.port_start,
                   port_end=sub.port_end, next_port=next_port)
    rc = torch.zeros(1, dtype=torch.int32, device=dev.device)
    dev.ext.subctx_upsert(dev.subctx, torch.from_numpy(np.frombuffer(
        bytearray(bytes(e)), dtype=np.uint8)).to(dev.device),
        abi.CTX_SET_NAT, rc)
    assert rc.cpu().tolist() == [0]
    cpu.dp.subnat[sub.private_ip].next_port = next_port


@pytest.fixture
def grid_cap():
    from bng_amd.dataplane.build import get_ext
    ext = get_ext(required=True)
    try:
        yield ext.set_pkt_grid_cap
    finally:
        ext.set_pkt_grid_cap(0)


# ------------------------------------------------------------------ device
def device_batch(dev, frames, stride=512):
    """Rows pre-filled with a sentinel past each frame."""
    import torch
    data = np.full((len(frames), stride), SENTINEL, dtype=np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    lens = np.array([len(f) for f in frames], dtype=np.uint16)
    d = torch.from_numpy(data).to(dev.device)
    assert d.data_ptr() % 16 == 0
    return d, torch.from_numpy(lens.view(np.int16)).to(dev.device)


def rows_of(d, frames):
    rows = d.cpu().numpy()
    out = []
    for i, f in enumerate(frames):
        past = rows[i, len(f):]
        assert (past == SENTINEL).all(), f"row {i}: written past the frame"
        out.append(rows[i, :len(f)].tobytes())
    return out


def device_egress(dev, frames, entry):
    """entry: "nat44" (stand-alone kernel), "uplink" (fused kernel) or
    "uplink-order" (fused, through a shuffled order tensor)."""
    import torch
    d, l = device_batch(dev, frames)
    if entry == "nat44":
        v = dev.nat44(d, l, egress=True, now_ns=NOW_NS)
    else:
        order = None
        if entry == "uplink-order":
            perm = list(range(len(frames)))
            random.Random(len(frames)).shuffle(perm)
            order = torch.from_numpy(np.array(perm, dtype=np.int32)) \
                .to(dev.device)
        v, ol = dev.uplink(d, l, now_ns=NOW_NS, now_sec=NOW_SEC, order=order)
        assert ol.cpu().numpy().view(np.uint16).tolist() == \
            [len(f) for f in frames]
    return v.cpu().tolist(), rows_of(d, frames)


def device_ingress(dev, frames, entry):
    d, l = device_batch(dev, frames)
    if entry == "nat44":
        v = dev.nat44(d, l, egress=False, now_ns=NOW_NS + MS)
    else:
        v = dev.downlink(d, l, now_ns=NOW_NS + MS)
    return v.cpu().tolist(), rows_of(d, frames)


def device_block(dev, ip):
    """The subscriber's bng_subctx entry, read back from the table."""
    raw = dev.subctx.cpu().numpy()
    rows = raw.view(np.uint32).reshape(-1, 16)
    hit = np.nonzero(rows[:, 0] == ip)[0]
    assert len(hit) == 1
    return abi.SubCtx.from_buffer_copy(rows[hit[0]].tobytes())


# ------------------------------------------------------------------ golden
def golden_egress(cpu, frames, fused):
    """[(verdict, bytes)] in batch order; fused = the uplink kernel's chain
    (antispoof, SNAT, ingress QoS)."""
    dp, out = cpu.dp, []
    for f in frames:
        fb = bytearray(f)
        if fused:
            v = dp.antispoof(bytes(fb))
            if v == FWD:
                v = dp.nat44_egress(fb)
            if v == FWD:
                v = dp.qos(bytes(f), "ingress")
        else:
            v = dp.nat44_egress(fb)
        out.append((v, bytes(fb)))
    return out


def golden_ingress(cpu, frames, fused):
    dp, out = cpu.dp, []
    dp.now_ns = NOW_NS + MS
    for f in frames:
        fb = bytearray(f)
        v = dp.nat44_ingress(fb)
        if fused and v == FWD:
            v = dp.qos(bytes(fb), "egress")
        out.append((v, bytes(fb)))
    dp.now_ns = NOW_NS
    return out


def stats_of(l, fused):
    st = {"nat": l.nat_get_stats()}
    if fused:
        st.update(dhcp=l.get_stats(), qos=l.qos_get_stats(),
                  antispoof=l.antispoof_get_stats())
    return st


# ------------------------------------------------------------------ checks
def port_of(frame):
    return wo.flow_fields(frame)[3]


def ports_of(entries, frames, sub):
    return [port_of(f) for e, f in zip(entries, frames) if e.sub == sub]


def session_keys(export):
    return sorted((int(r["src_ip"]), int(r["dst_ip"]), int(r["src_port"]),
                   int(r["dst_port"]), int(r["protocol"]), int(r["nat_ip"]))
                  for r in export)


def creates(log, sub=None):
    return [r for r in log if r["event_type"] == abi.LOG_SESSION_CREATE and
            (sub is None or r["private_ip"] == sub.private_ip)]


def no_exhaustion(stats, log):
    assert stats["port_exhaustion"] == 0 and stats["packets_dropped"] == 0
    assert not [r for r in log
                if r["event_type"] == abi.LOG_PORT_EXHAUSTION]


def check_frames(entries, verdicts, frames):
    """Every row forwarded and a legal translation into its subscriber's
    block that the receiver accepts, byte for byte the datagram rebuilt the
    sender's way with the port this row got."""
    for i, (e, v, got) in enumerate(zip(entries, verdicts, frames)):
        where = f"row {i} ({e.cls}, proto {e.frame[23]}, len {len(e.frame)})"
        assert v == FWD, where
        s = e.sub
        assert wo.verify_translation(e.frame, got, "egress", s.public_ip,
                                     (s.port_start, s.port_end)) == [], where
        assert wo.verify_frame(got) == [], where
        assert got == wo.expected_egress(e.frame, s.public_ip,
                                         port_of(got)), where


def check_block(dev, cpu, sub, rotor=True):
    """The block's counters against the golden's; the rotor inside the
    block always, and equal to the sequential model's unless the number of
    skipped positions depends on lane order (rotor=False)."""
    got, want = device_block(dev, sub.private_ip), \
        cpu.dp.subnat[sub.private_ip]
    assert sub.port_start <= got.next_port <= sub.port_end
    assert sub.port_start <= want.next_port <= sub.port_end
    if rotor:
        assert got.next_port == want.next_port
    assert (got.sessions_active, got.sessions_total) == \
        (want.sessions_active, want.sessions_total)
    return got


def check_burst(dev, cpu, sub, entries, out, fused, n_sessions):
    """Step B's assertions on one batch that holds a burst of `sub` to ONE
    destination, no more flows than the block has ports."""
    v, frames = out
    gold = golden_egress(cpu, [e.frame for e in entries], fused)
    assert [g[0] for g in gold] == [FWD] * len(entries)
    check_frames(entries, v, frames)
    mine = ports_of(entries, frames, sub)
    want = ports_of(entries, [g[1] for g in gold], sub)
    print(f"ports {sorted(mine)}\ngolden {sorted(want)}")
    assert sorted(mine) == sorted(want)
    assert len(set(mine)) == len(mine)
    assert all(sub.port_start <= p <= sub.port_end for p in mine)
    # the crowd: first flow of a fresh block each, whatever the order
    assert [port_of(f) for e, f in zip(entries, frames) if e.sub != sub] == \
        [e.sub.port_start for e in entries if e.sub != sub]
    assert stats_of(dev, fused) == stats_of(cpu, fused)
    log, glog = dev.drain_nat_log(), cpu.drain_nat_log()
    no_exhaustion(dev.nat_get_stats(), log)
    check_block(dev, cpu, sub)
    # one live session per flow, each burst session on a port of its own
    exp, gexp = dev.export_nat_sessions(), cpu.export_nat_sessions()
    assert len(exp) == n_sessions
    assert session_keys(exp) == session_keys(gexp)
    dest = wo.flow_fields(next(e.frame for e in entries if e.sub == sub))[1]
    burst_ports = [int(r["nat_port"]) for r in exp
                   if r["src_ip"] == sub.private_ip and r["dst_ip"] == dest]
    assert sorted(burst_ports) == sorted(mine)
    # the compliance log: one SESSION_CREATE per flow, no two records of
    # the burst with the same public endpoint towards the destination
    assert len(creates(log)) == len(creates(glog)) == len(entries)
    recs = [(r["public_ip"], r["public_port"], r["dest_ip"], r["dest_port"],
             r["protocol"]) for r in creates(log, sub)]
    assert len(recs) == len(mine) and len(set(recs)) == len(recs)
    assert sorted(r[1] for r in recs) == sorted(mine)
    assert {r["subscriber_id"] for r in creates(log, sub)} == {SUBJECT_ID}
    return [g[1] for g in gold]


def check_round_trip(dev, cpu, entries, translated, gold_translated, entry):
    """Step C: one reply per translated frame back through DNAT.  Which
    flow of the burst got which port differs between device and model, so
    each side answers its own translation (the same reply but for the
    port) and the burst's replies are judged by the oracle alone."""
    fused = entry != "nat44"
    rng, grng = random.Random(7), random.Random(7)
    replies = [wo.build_reply(t, rng) for t in translated]
    v, got = device_ingress(dev, replies, entry)
    gold = golden_ingress(cpu, [wo.build_reply(t, grng)
                                for t in gold_translated], fused)
    for i, (e, r, g) in enumerate(zip(entries, replies, got)):
        where = f"reply to row {i} ({e.cls}, proto {e.frame[23]})"
        assert wo.verify_frame(r) == [], where
        assert v[i] == gold[i][0] == FWD, where
        assert wo.audit_ingress(e, r, g) == [], where
        if e.cls == "other":
            assert g == gold[i][1], where + ": differs from golden"
    assert stats_of(dev, fused) == stats_of(cpu, fused)
    assert dev.nat_get_stats()["packets_dnat"] == len(replies)


# ---------------------------------------------------------------- scenarios
def abc_scenario(block, n_total):
    """(subject, subscribers, step A's entries, step B's entries)."""
    sub = subject(block)
    m = block[1] - block[0] + 1
    a = burst(sub, 0, PRE, DEST_A)
    b = interleave(burst(sub, 3000, m, DEST_B), n_total)
    return sub, with_others([sub], n_total - m), a, b


def overflow_scenario(block, n_total, m=40):
    """Step D: more flows than ports, one destination."""
    sub = subject(block)
    return sub, with_others([sub], n_total - m), \
        interleave(burst(sub, 6000, m, DEST_B), n_total)


def parity_scenario(near_end):
    """Step E: two subscribers on 1024-port blocks, 64 flows each, one with
    even source ports and one with odd, rows alternating.  near_end puts
    both rotors 40 positions before the end, so the burst wraps."""
    subs = [subject(WIDE, 0), subject(WIDE, 1)]
    ent = []
    for j in range(64):
        for k, s in enumerate(subs):
            ent.append(flow(s, j, DEST_B, proto=wo.PROTOS[j % 3],
                            sport=40000 + 2 * j + k))
    rotor = WIDE[1] - 40 if near_end else None
    return subs, [(s, SUBJECT_ID) for s in subs], ent, rotor


def eim_scenario():
    """Step F: one endpoint, then 64 flows from it to 64 destinations."""
    sub = subject(LOW16)
    first = [flow(sub, 0, DEST_A, proto=wo.UDP, sport=41000)]
    fan = [flow(sub, 1 + j, (DEST_B[0] + 1 + j, 53), proto=wo.UDP,
                sport=41000) for j in range(64)]
    return sub, [(sub, SUBJECT_ID)], first, fan


ABC_SHAPES = [(blk, n, cap) for blk in (LOW16, TOP16)
              for n, cap in ((16, 0), (64, 0), (65, 0), (256 + 37, 1))] + \
             [(WIDE, 1024 + 37, 0), (WIDE, 1024 + 37, 1)]
ENTRIES = ["nat44", "uplink", "uplink-order"]
OVERFLOW_SHAPES = [(blk, n, cap) for blk in (LOW16, TOP16)
                   for n, cap in ((40, 0), (256 + 37, 1))]


def shape_id(s):
    return f"{s[0][0]}-{s[0][1]}-n{s[1]}-cap{s[2]}"


# ===================================================================== CPU
def test_golden_handles_every_scenario():
    """The golden model alone on every scenario's frames: the invariants of
    steps B, D and E hold on the reference's own output."""
    for blk, n, _cap in ABC_SHAPES:
        sub, subs, a, b = abc_scenario(blk, n)
        for fused in (False, True):
            cpu = golden_launcher(subs)
            out = golden_egress(cpu, [e.frame for e in a], fused)
            assert [port_of(f) for _v, f in out] == \
                list(range(blk[0], blk[0] + PRE))
            assert cpu.dp.subnat[sub.private_ip].next_port == blk[0] + PRE
            out = golden_egress(cpu, [e.frame for e in b], fused)
            assert [v for v, _f in out] == [FWD] * n
            check_frames(b, [v for v, _f in out], [f for _v, f in out])
            ports = ports_of(b, [f for _v, f in out], sub)
            assert sorted(ports) == list(range(blk[0], blk[1] + 1))
            no_exhaustion(cpu.nat_get_stats(), cpu.drain_nat_log())
            assert cpu.dp.subnat[sub.private_ip].next_port == blk[0] + PRE
            assert len(cpu.export_nat_sessions()) == PRE + n
    for blk, n, _cap in OVERFLOW_SHAPES:
        sub, subs, d = overflow_scenario(blk, n)
        cpu = golden_launcher(subs)
        out = golden_egress(cpu, [e.frame for e in d], False)
        assert DROP not in [v for v, _f in out]
        turns = Counter(ports_of(d, [f for _v, f in out], sub))
        assert sorted(turns) == list(range(blk[0], blk[1] + 1))
        assert set(turns.values()) == {2, 3} and sum(turns.values()) == 40
        no_exhaustion(cpu.nat_get_stats(), cpu.drain_nat_log())
    for near_end in (False, True):
        subs, table, ent, rotor = parity_scenario(near_end)
        cpu = golden_launcher(table, abi.NAT_FLAG_EIM | abi.NAT_FLAG_PARITY)
        if rotor is not None:
            for s in subs:
                cpu.dp.subnat[s.private_ip].next_port = rotor
        out = golden_egress(cpu, [e.frame for e in ent], False)
        assert [v for v, _f in out] == [FWD] * len(ent)
        for k, s in enumerate(subs):
            ports = ports_of(ent, [f for _v, f in out], s)
            assert len(set(ports)) == 64
            assert all(WIDE[0] <= p <= WIDE[1] and p & 1 == k for p in ports)
            assert WIDE[0] <= cpu.dp.subnat[s.private_ip].next_port <= WIDE[1]
            if near_end:                 # both sides of the wrap
                assert min(ports) < WIDE[0] + 100 < WIDE[1] - 41 < max(ports)
    sub, table, first, fan = eim_scenario()
    cpu = golden_launcher(table)
    out = golden_egress(cpu, [e.frame for e in first + fan], False)
    assert [port_of(f) for _v, f in out] == [LOW16[0]] * 65
    assert cpu.nat_get_stats()["eim_hits"] == 64


# ===================================================================== GPU
@gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ABC_SHAPES, ids=shape_id)
def test_burst_to_one_destination(shape, entry, grid_cap):
    """Steps A to C.  A: ten flows bring the rotor ten ports in, and the
    device's next_port is the model's.  B: a burst as large as the block
    wraps the rotor inside one batch; every port of the block goes out
    exactly once.  C: every reply comes back to the flow that sent."""
    blk, n_total, cap = shape
    fused = entry != "nat44"
    sub, subs, a, b = abc_scenario(blk, n_total)
    # both parsers meet every protocol: ihl 5 and 48 bytes or more on an
    # aligned row (the register window), and a header with options
    for proto in wo.PROTOS:
        mine = [e.frame for e in b if e.sub == sub and e.frame[23] == proto]
        assert any(f[14] == 0x45 and len(f) >= 48 for f in mine)
        assert any(f[14] == 0x46 for f in mine)
    dev, cpu = make_pair(subs, log2=12 if blk == WIDE else 10)
    # A
    out = device_egress(dev, [e.frame for e in a], entry)
    gold = golden_egress(cpu, [e.frame for e in a], fused)
    assert out[0] == [g[0] for g in gold] == [FWD] * PRE
    assert sorted(map(port_of, out[1])) == \
        sorted(port_of(g[1]) for g in gold)
    assert check_block(dev, cpu, sub).next_port == blk[0] + PRE
    dev.drain_nat_log()
    cpu.drain_nat_log()
    # B
    grid_cap(cap)
    out = device_egress(dev, [e.frame for e in b], entry)
    grid_cap(0)
    gold_out = check_burst(dev, cpu, sub, b, out, fused,
                           n_sessions=PRE + n_total)
    # C
    check_round_trip(dev, cpu, b, out[1], gold_out, entry)


@gpu
@pytest.mark.parametrize("entry", ["nat44", "uplink"])
@pytest.mark.parametrize("shape", OVERFLOW_SHAPES, ids=shape_id)
def test_more_flows_than_ports_reuse_not_exhaustion(shape, entry, grid_cap):
    """Step D: 40 new flows on 16 ports.  Reuse after a full turn is the
    reference's design; it must stay reuse: the multiset of ports is the
    sequential model's (each port two or three times), none outside the
    block, nothing dropped."""
    blk, n_total, cap = shape
    fused = entry != "nat44"
    sub, subs, d = overflow_scenario(blk, n_total)
    dev, cpu = make_pair(subs)
    grid_cap(cap)
    v, frames = device_egress(dev, [e.frame for e in d], entry)
    grid_cap(0)
    gold = golden_egress(cpu, [e.frame for e in d], fused)
    assert v == [g[0] for g in gold] == [FWD] * n_total
    check_frames(d, v, frames)
    got = Counter(ports_of(d, frames, sub))
    want = Counter(ports_of(d, [g[1] for g in gold], sub))
    print(f"ports {sorted(got.items())}\ngolden {sorted(want.items())}")
    assert got == want
    assert set(got.values()) == {2, 3}
    assert all(blk[0] <= p <= blk[1] for p in got)
    assert stats_of(dev, fused) == stats_of(cpu, fused)
    no_exhaustion(dev.nat_get_stats(), dev.drain_nat_log())
    check_block(dev, cpu, sub)
    assert session_keys(dev.export_nat_sessions()) == \
        session_keys(cpu.export_nat_sessions())


@gpu
@pytest.mark.parametrize("entry", ["nat44", "uplink"])
@pytest.mark.parametrize("near_end", [False, True], ids=["start", "wrap"])
def test_parity_burst(near_end, entry):
    """Step E: with one parity wanted per block, the ports handed out are
    the first 64 positions of that parity from the rotor on, whatever the
    lane order; how many positions were skipped is not, so next_port is
    only checked to lie in the block."""
    fused = entry != "nat44"
    subs, table, ent, rotor = parity_scenario(near_end)
    dev, cpu = make_pair(table, abi.NAT_FLAG_EIM | abi.NAT_FLAG_PARITY)
    if rotor is not None:
        for s in subs:
            set_rotor(dev, cpu, s, SUBJECT_ID, rotor)
    v, frames = device_egress(dev, [e.frame for e in ent], entry)
    gold = golden_egress(cpu, [e.frame for e in ent], fused)
    assert v == [g[0] for g in gold] == [FWD] * len(ent)
    check_frames(ent, v, frames)
    for k, s in enumerate(subs):
        got = ports_of(ent, frames, s)
        want = ports_of(ent, [g[1] for g in gold], s)
        print(f"sub {k}: ports {sorted(got)}\ngolden {sorted(want)}")
        assert len(set(got)) == 64 and set(got) == set(want)
        assert all(WIDE[0] <= p <= WIDE[1] and p & 1 == k for p in got)
        check_block(dev, cpu, s, rotor=False)
    assert stats_of(dev, fused) == stats_of(cpu, fused)
    no_exhaustion(dev.nat_get_stats(), dev.drain_nat_log())


@gpu
@pytest.mark.parametrize("entry", ["nat44", "uplink"])
def test_eim_hits_across_batches_take_no_port(entry):
    """Step F: an endpoint mapped in one batch serves 64 new flows of the
    next from the same ip:port to 64 destinations: all leave on its
    external port, each counts an EIM hit, and the rotor does not move."""
    fused = entry != "nat44"
    sub, table, first, fan = eim_scenario()
    dev, cpu = make_pair(table)
    v, frames = device_egress(dev, [e.frame for e in first], entry)
    golden_egress(cpu, [e.frame for e in first], fused)
    assert v == [FWD] and port_of(frames[0]) == LOW16[0]
    before = dev.nat_get_stats()
    rotor = check_block(dev, cpu, sub).next_port
    assert rotor == LOW16[0] + 1
    v, frames = device_egress(dev, [e.frame for e in fan], entry)
    gold = golden_egress(cpu, [e.frame for e in fan], fused)
    assert v == [g[0] for g in gold] == [FWD] * 64
    check_frames(fan, v, frames)
    assert [port_of(f) for f in frames] == [LOW16[0]] * 64
    st = dev.nat_get_stats()
    assert st["eim_hits"] - before["eim_hits"] == 64
    assert st["eim_misses"] == before["eim_misses"]
    assert stats_of(dev, fused) == stats_of(cpu, fused)
    assert check_block(dev, cpu, sub).next_port == rotor
    assert session_keys(dev.export_nat_sessions()) == \
        session_keys(cpu.export_nat_sessions())
