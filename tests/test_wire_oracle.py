"""The receiver-side oracle (wire_oracle.py), and the golden model under it.

The GPU suite compares the kernels with `GoldenDataplane`, a port of the
same incremental-checksum algorithm.  Here the golden model itself is put
under an oracle that shares nothing with it:

  * the oracle accepts correct translations and reports every single-field
    mutation of one,
  * the golden model's SNAT and DNAT pass the whole seeded corpus,
  * the corpus is sensitive: with the checksum arithmetic broken in one of
    three ways, or a parser fix taken out, the oracle flags it,
  * every corpus frame is checked by the path its class prescribes, and most
    translated frames are checked from scratch.
"""
import collections
import struct

import pytest

import wire_oracle as wo
from bng_amd.dataplane import abi
from bng_amd.dataplane.golden import FWD, PASS, GoldenDataplane
from bng_amd.dataplane.launcher import GoldenLauncher

NOW_NS = 1_700_000_000 * 10**9

WANT_VERDICT = {wo.SCRATCH: FWD, wo.DELTA: FWD, wo.UNTOUCHED_FWD: FWD,
                wo.UNTOUCHED_PASS: PASS}

CLASSES = {
    "payload_len", "edge_port", "block_1024", "block_one_port_65535",
    "public_edge", "private_zero_low", "land_0000", "land_ffff", "land_0001",
    "land_fffe", "csum_ffff_in", "icmp_double_carry", "udp_csum_none_in",
    "len_branch", "short_l4", "ip_options", "eth_padding", "bad_l4_csum_in",
    "first_fragment", "frag_nonfirst", "bad_ihl", "bad_version", "icmp_error",
    "icmp_query", "random"}


@pytest.fixture(scope="module")
def corpus():
    return wo.build_corpus()


def golden_for(corpus):
    cpu = GoldenLauncher()
    cpu.dp.now_ns = NOW_NS
    for e in corpus.entries:
        s = e.sub
        cpu.add_subscriber_nat(s.private_ip, s.public_ip, s.port_start,
                               s.port_end, subscriber_id=1)
    return cpu


def golden_egress(corpus):
    """(launcher, [(verdict, output)]) of the golden SNAT over the corpus."""
    cpu = golden_for(corpus)
    out = []
    for e in corpus.entries:
        fb = bytearray(e.frame)
        out.append((cpu.dp.nat44_egress(fb), bytes(fb)))
    return cpu, out


def egress_report(corpus, out):
    """{class: [problem, ...]} and {class: Counter(path)}."""
    problems = collections.defaultdict(list)
    paths = collections.defaultdict(collections.Counter)
    for i, (e, (v, after)) in enumerate(zip(corpus.entries, out)):
        bad = wo.audit_egress(e, after)
        if v != WANT_VERDICT[e.check]:
            bad = bad + ["verdict %d, want %d" % (v, WANT_VERDICT[e.check])]
        paths[e.cls][e.check] += 1
        problems[e.cls] += ["frame %d: %s" % (i, b) for b in bad]
    return {k: v for k, v in problems.items() if v}, paths


# ------------------------------------------------------------- the corpus
def test_every_class_is_there(corpus):
    got = corpus.classes()
    assert set(got) == CLASSES
    assert all(got[c] for c in CLASSES)
    assert corpus.pairs() == wo.corpus()            # seeded: reproducible
    assert 200 <= len(corpus.entries) <= 600


def test_corpus_holds_what_its_classes_claim(corpus):
    cl = corpus.classes()

    def lens(c, proto=None):
        return sorted(len(e.frame) for e in cl[c]
                      if proto is None or e.frame[23] == proto)
    assert lens("len_branch", wo.UDP) == list(range(42, 50))
    assert lens("len_branch", wo.ICMP) == list(range(42, 50))
    assert lens("len_branch", wo.TCP) == [54, 55]
    assert lens("short_l4") == [41, 41, 53, 93]
    assert 94 in lens("ip_options", wo.TCP)
    assert {e.frame[14] & 0xF for e in cl["ip_options"]} == {6, 7, 15}
    assert {e.frame[14] for e in cl["bad_ihl"]} == set(range(0x40, 0x45))
    assert {e.frame[14] for e in cl["bad_version"]} == {0x55, 0x65}
    for e in cl["eth_padding"]:
        assert len(e.frame) > 14 + struct.unpack_from(">H", e.frame, 16)[0]
    assert all(struct.unpack_from(">H", e.frame, 20)[0] == 0x2000
               for e in cl["first_fragment"])
    ff = {struct.unpack_from(">H", e.frame, 20)[0] for e in cl["frag_nonfirst"]}
    assert all(f & 0x1FFF for f in ff) and \
        {bool(f & 0x2000) for f in ff} == {False, True}
    assert {e.frame[34] for e in cl["icmp_error"]} == {3, 5, 11}
    assert {e.frame[34] for e in cl["icmp_query"]} == {13, 17}
    assert {e.sub.public_ip for e in cl["public_edge"]} == \
        {0xFFFF0001, 0x0100FFFF}
    assert all(e.sub.private_ip & 0xFFFF == 0 for e in cl["private_zero_low"])
    assert all((e.sub.port_start, e.sub.port_end) == (65535, 65535)
               for e in cl["block_one_port_65535"])
    for c in ("payload_len", "edge_port", "land_0000", "land_ffff",
              "land_0001", "land_fffe", "eth_padding", "bad_l4_csum_in",
              "first_fragment", "frag_nonfirst", "bad_ihl", "bad_version"):
        assert {e.frame[23] for e in cl[c]} == {wo.TCP, wo.UDP, wo.ICMP}, c
    # well-formed on arrival, except where the class says otherwise
    for e in corpus.entries:
        if e.check == wo.SCRATCH:
            assert wo.verify_frame(e.frame) == [], e.cls
    for e in cl["bad_l4_csum_in"]:
        assert len(wo.verify_frame(e.frame)) == 1
    # the landing values, on the sender-side rebuild of the output
    for cls, want in (("land_0000", {0x0000, 0xFFFF}), ("land_0001", {1}),
                      ("land_fffe", {0xFFFE}), ("land_ffff", {0, 0xFFFF})):
        for e in cl[cls]:
            out = wo.expected_egress(e.frame, e.sub.public_ip,
                                     e.sub.port_start)
            lay = wo.layout(out)
            ck = struct.unpack_from(
                ">H", out, lay.l4 + wo.CSUM_AT[lay.proto])[0]
            assert ck in want, (cls, hex(ck))
            assert (ck == 0xFFFF) == (lay.proto == wo.UDP and want != {1}
                                      and want != {0xFFFE})
    for e in cl["land_ffff"] + cl["csum_ffff_in"]:
        lay = wo.layout(e.frame)
        assert struct.unpack_from(
            ">H", e.frame, lay.l4 + wo.CSUM_AT[lay.proto])[0] == 0xFFFF


# --------------------------------------------------- the oracle's own teeth
def flip(frame, at, bit=0x10):
    out = bytearray(frame)
    out[at] ^= bit
    return bytes(out)


def mutations(before, good):
    """(name, mutated output) for every single-field mutation the frame
    has room for."""
    lay = wo.layout(before)
    l4, proto = lay.l4, lay.proto
    id_at, ck_at = l4 + wo.SRC_ID_AT[proto], l4 + wo.CSUM_AT[proto]
    body = l4 + wo.L4_HDR[proto]
    if lay.end > body:
        yield "payload bit", flip(good, body + (lay.end - body) // 2)
    if lay.ihl > 20:
        yield "option bit", flip(good, 34 + (lay.ihl - 20) // 2)
    if len(before) > lay.end:
        yield "padding bit", flip(good, len(before) - 1)
    yield "L4 checksum bit", flip(good, ck_at + 1)
    yield "IP checksum bit", flip(good, 24)
    yield "port bit", flip(good, id_at + 1, 0x01)
    if before[id_at:id_at + 2] != good[id_at:id_at + 2]:
        yield "port left alone", good[:id_at] + before[id_at:id_at + 2] + \
            good[id_at + 2:]
    yield "ethernet bit", flip(good, 3)
    yield "destination bit", flip(good, 31)


def test_oracle_accepts_good_and_reports_every_mutation(corpus):
    """The correct translation of each well-formed frame, rebuilt the
    sender's way, is clean; every single-field mutation of it is reported
    by verify_translation.  The delta-only classes take the golden model's
    output, once that is clean, as the correct one."""
    _cpu, out = golden_egress(corpus)
    seen = collections.Counter()
    for e, (_v, gold) in zip(corpus.entries, out):
        if e.check == wo.SCRATCH:
            good = wo.expected_egress(e.frame, e.sub.public_ip,
                                      e.sub.port_start)
        elif e.check == wo.DELTA:
            good = gold
        else:
            assert wo.untouched(e.frame, e.frame) == []
            assert wo.untouched(e.frame, flip(e.frame, len(e.frame) - 1))
            assert wo.untouched(e.frame, flip(e.frame, 14))
            continue
        rng = (e.sub.port_start, e.sub.port_end)
        assert wo.verify_translation(e.frame, good, "egress",
                                     e.sub.public_ip, rng) == [], e.cls
        assert wo.audit_egress(e, good) == [], e.cls
        for name, bad in mutations(e.frame, good):
            # UDP without a checksum: no sum speaks for the port, another
            # port of the block is a legal translation; only the audit,
            # which knows the block is fresh, reports it
            assert wo.verify_translation(e.frame, bad, "egress",
                                         e.sub.public_ip, rng) or \
                (e.cls == "udp_csum_none_in" and name == "port bit"), \
                "%s not reported (%s)" % (name, e.cls)
            assert wo.audit_egress(e, bad)
            seen[name] += 1
        # wrong public address, port outside the block
        assert wo.verify_translation(e.frame, good, "egress",
                                     e.sub.public_ip ^ 1, rng)
        assert wo.verify_translation(e.frame, good, "egress", e.sub.public_ip,
                                     (e.sub.port_start + 1, 65535)) or \
            e.sub.port_start == 65535
    assert all(seen[k] for k in ("payload bit", "option bit", "padding bit",
                                 "L4 checksum bit", "IP checksum bit",
                                 "port bit", "port left alone"))


def test_verify_frame_reports_each_rule():
    sub_mac = bytes.fromhex("aabb00000001")
    ok = wo.build_frame(wo.UDP, 0x0A000001, wo.DST_IP, src_mac=sub_mac,
                        sport=5, dport=6, payload=b"abc")
    assert wo.verify_frame(ok) == []
    assert wo.verify_frame(flip(ok, 14, 0x10))          # version 5
    assert wo.verify_frame(ok[:14] + b"\x44" + ok[15:])  # ihl 4
    assert wo.verify_frame(ok[:14] + b"\x4f" + ok[15:])  # header past frame
    assert wo.verify_frame(flip(ok, 22))                 # ttl: header sum
    assert wo.verify_frame(flip(ok, 43))                 # payload: UDP sum
    assert wo.verify_frame(ok[:12] + b"\x86\xdd" + ok[14:])
    none = wo.build_frame(wo.UDP, 0x0A000001, wo.DST_IP, src_mac=sub_mac,
                          sport=5, dport=6, payload=b"abc", l4_csum=0)
    assert wo.verify_frame(none) == [] and wo.verify_frame(flip(none, 43)) == []
    for proto in (wo.TCP, wo.ICMP):
        f = wo.build_frame(proto, 0x0A000001, wo.DST_IP, src_mac=sub_mac,
                           payload=b"abcde", pad_to=64)
        assert wo.verify_frame(f) == []
        assert wo.verify_frame(flip(f, len(f) - 1)) == []   # padding
        assert wo.verify_frame(flip(f, 34))
    # both representations of zero verify
    c = wo.Corpus(1)
    f = c.add_landing("x", wo.TCP, 0, solve_input=True)
    lay = wo.layout(f)
    assert f[lay.l4 + 16:lay.l4 + 18] == b"\xff\xff"
    assert wo.verify_frame(f) == []
    assert wo.verify_frame(f[:lay.l4 + 16] + b"\x00\x00" +
                           f[lay.l4 + 18:]) == []
    assert wo.verify_frame(f[:lay.l4 + 16] + b"\x00\x01" + f[lay.l4 + 18:])


# ------------------------------------------------ the golden model under it
def test_golden_snat_passes_the_corpus(corpus):
    cpu, out = golden_egress(corpus)
    problems, paths = egress_report(corpus, out)
    assert problems == {}
    # coverage conditions
    total = collections.Counter()
    for cls, c in paths.items():
        total.update(c)
        if wo.DELTA in c:
            assert cls in ("first_fragment", "bad_l4_csum_in")
    translated = total[wo.SCRATCH] + total[wo.DELTA]
    assert sum(total.values()) == len(corpus.entries)
    assert total[wo.SCRATCH] * 4 >= translated * 3
    scratch_l4 = sum(wo.from_scratch_possible(e.frame)
                     for e in corpus.entries if e.check == wo.SCRATCH)
    assert scratch_l4 * 4 >= translated * 3
    st = cpu.nat_get_stats()
    assert st["packets_snat"] == st["sessions_created"] == translated
    assert st["packets_passed"] == total[wo.UNTOUCHED_PASS]
    assert st["packets_dropped"] == 0
    for cls in sorted(paths):
        print("%-22s %s" % (cls, dict(paths[cls])))


def test_golden_dnat_passes_the_replies(corpus):
    cpu, out = golden_egress(corpus)
    before = cpu.nat_get_stats()
    replies = wo.build_replies(corpus.entries, [o[1] for o in out])
    assert len(replies) == before["packets_snat"]
    for i, reply in replies:
        assert wo.verify_frame(reply) == []
        fb = bytearray(reply)
        assert cpu.dp.nat44_ingress(fb) == FWD
        bad = wo.audit_ingress(corpus.entries[i], reply, bytes(fb))
        assert bad == [], (corpus.entries[i].cls, bad)
    assert cpu.nat_get_stats()["packets_dnat"] == len(replies)


def test_golden_ingress_leaves_fragments_and_errors_alone(corpus):
    """What the egress side hands to the host, and malformed headers, come
    back untouched on ingress too, with FWD and no counter moved — also
    when their bytes 'match' a live session."""
    cpu, _out = golden_egress(corpus)
    before = cpu.nat_get_stats()
    for e in corpus.entries:
        if e.check in (wo.UNTOUCHED_FWD, wo.UNTOUCHED_PASS):
            fb = bytearray(e.frame)
            assert cpu.dp.nat44_ingress(fb) == FWD
            assert wo.untouched(e.frame, fb) == []
    after = cpu.nat_get_stats()
    # short frames of a known protocol count nothing either
    assert after == before


# -------------------------------------------------- the corpus's own teeth
def fold_once16(csum, old, new):
    s = (~csum) & 0xFFFF
    s += (~old & 0xFFFF) + (new & 0xFFFF)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def no_high_half_of_old(csum, old, new):
    s = (~csum) & 0xFFFF
    s += (~old & 0xFFFF)
    s += (new & 0xFFFF) + (new >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def test_single_carry_fold_is_flagged(corpus, monkeypatch):
    monkeypatch.setattr(GoldenDataplane, "_upd_csum16",
                        staticmethod(fold_once16))
    problems, _ = egress_report(corpus, golden_egress(corpus)[1])
    assert "icmp_double_carry" in problems


def test_dropped_high_half_is_flagged(corpus, monkeypatch):
    monkeypatch.setattr(GoldenDataplane, "_upd_csum",
                        staticmethod(no_high_half_of_old))
    problems, _ = egress_report(corpus, golden_egress(corpus)[1])
    assert {"payload_len", "random", "first_fragment",
            "bad_l4_csum_in"} <= set(problems)


def test_udp_zero_left_as_zero_is_flagged(corpus, monkeypatch):
    """A rewrite without the `0 -> 0xFFFF` step.  The step sits inside
    nat44_egress, so the break is put behind it: the incremental update
    never yields 0xFFFF itself (its accumulator is never zero), so a UDP
    checksum that leaves as 0xFFFF was 0 before that step."""
    real = GoldenDataplane.nat44_egress

    def without_the_step(self, frame):
        v = real(self, frame)
        lay = wo.layout(frame)
        if not isinstance(lay, str) and lay.proto == wo.UDP and \
                not lay.frag_off and len(frame) >= lay.l4 + 8 and \
                frame[lay.l4 + 6:lay.l4 + 8] == b"\xff\xff":
            frame[lay.l4 + 6:lay.l4 + 8] = b"\x00\x00"
        return v
    monkeypatch.setattr(GoldenDataplane, "nat44_egress", without_the_step)
    problems, _ = egress_report(corpus, golden_egress(corpus)[1])
    assert set(problems) == {"land_0000", "land_ffff"}
    assert all("UDP" in p for v in problems.values() for p in v)


def test_accepting_short_ihl_is_flagged(corpus, monkeypatch):
    """The parser fix taken out again: the malformed classes fail."""
    monkeypatch.setattr(GoldenDataplane, "_ipv4_header_ok",
                        staticmethod(lambda frame, off: True))
    problems, _ = egress_report(corpus, golden_egress(corpus)[1])
    assert "bad_ihl" in problems
