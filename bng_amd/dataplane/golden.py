"""CPU golden-model dataplane.

Packet-exact reference implementation of the four dataplane kernels:

  * DHCP fast path   (ref bpf/dhcp_fastpath.c:619-813)
  * NAT44 SNAT/DNAT  (ref bpf/nat44.c:565-948)
  * QoS token bucket (ref bpf/qos_ratelimit.c:126-222)
  * Antispoof uRPF   (ref bpf/antispoof.c:189-293)

Every HIP kernel is differential-tested against this model on random packet
batches (tests/test_kernels_gpu.py), the analog of the reference testing its
BPF programs through the kernel verifier + unit tests.

Reference quirks are preserved deliberately where the control plane depends
on them (e.g. antispoof's binding+LOOSE fallthrough, the EIM port-collision
heuristic); deviations are design upgrades shared by golden model and HIP
kernel alike (full TLV option scan instead of the reference's fixed-offset
verifier workaround, dhcp_fastpath.c:216-250).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from . import abi
from .packets import (ETH_P_8021AD, ETH_P_8021Q, ETH_P_IP, ETH_P_IPV6,
                      ipv4_checksum)

# verdicts
PASS, TX, DROP, FWD = abi.PASS, abi.TX, abi.DROP, abi.FWD


# ------------------------------------------------------------- table rows
@dataclass
class SubRecord:
    pool_id: int
    allocated_ip: int          # network-order u32
    lease_expiry: int          # unix seconds
    vlan_id: int = 0
    client_class: int = 0
    flags: int = 0


@dataclass
class PoolRecord:
    network: int
    prefix_len: int
    gateway: int
    dns_primary: int = 0
    dns_secondary: int = 0
    lease_time: int = 3600


@dataclass
class NatSessionRec:
    nat_ip: int
    nat_port: int              # network order
    orig_port: int             # network order
    orig_ip: int
    dest_ip: int
    dest_port: int
    state: int = abi.NAT_NEW
    is_hairpin: int = 0
    last_seen: int = 0
    created: int = 0
    packets_out: int = 0
    packets_in: int = 0
    bytes_out: int = 0
    bytes_in: int = 0
    protocol: int = 0


@dataclass
class EimRec:
    external_ip: int
    external_port: int         # HOST order (ref eim_mapping nat44.c:112-120)
    created: int = 0
    last_used: int = 0
    ref_count: int = 1
    flags: int = 0


@dataclass
class SubnatRec:
    public_ip: int
    port_start: int
    port_end: int
    next_port: int
    subscriber_id: int = 0
    sessions_active: int = 0
    sessions_total: int = 0
    bytes_out: int = 0
    bytes_in: int = 0
    ports_in_use: int = 0
    allocated_at: int = 0


@dataclass
class QosBucketRec:
    rate_bps: int
    burst_bytes: int
    tokens: int = 0
    last_update: int = 0
    priority: int = 0


@dataclass
class BindingRec:
    ipv4_addr: int = 0
    ipv4_valid: int = 0
    ipv6_addr: bytes = b"\x00" * 16
    ipv6_valid: int = 0
    mode: int = abi.AS_DISABLED


@dataclass
class PppoeSessRec:
    mac: int                   # client MAC as u64 (abi.mac_to_u64)
    ip: int                    # subscriber IPv4, host int of the BE field
    mru: int = 1492


@dataclass
class AcctRec:
    """Per-subscriber traffic counters (bng_acct_entry without its key)."""
    up_bytes: int = 0
    up_pkts: int = 0
    down_bytes: int = 0
    down_pkts: int = 0
    up_drop_pkts: int = 0
    down_drop_pkts: int = 0
    last_seen: int = 0


# ICMP types that carry an id at bytes 4..5: echo, timestamp, information
# and address-mask, request and reply.  Every other type is an error or a
# redirect, whose bytes 4..7 mean something else.
ICMP_QUERY_TYPES = frozenset((0, 8, 13, 14, 15, 16, 17, 18))

DEFAULT_PRIVATE_RANGES = [
    # is_private_ip inline ranges, ref nat44.c:340-363
    (0x0A000000, 0xFF000000),                    # 10.0.0.0/8
    (0xAC100000, 0xFFF00000),                    # 172.16.0.0/12
    (0xC0A80000, 0xFFFF0000),                    # 192.168.0.0/16
    (0x64400000, 0xFFC00000),                    # 100.64.0.0/10 CGNAT
]


class GoldenDataplane:
    """Semantic reference for the GPU dataplane; one instance = one shard."""

    def __init__(self, now_ns: int = 0):
        self.now_ns = now_ns
        # DHCP fast path tables
        self.subscribers: Dict[int, SubRecord] = {}   # tagged u64 key
        self.pools: Dict[int, PoolRecord] = {}
        self.server_mac = b"\x00" * 6
        self.server_ip = 0
        self.dhcp_stats = [0] * abi.DHCP_NSTATS
        # NAT tables
        self.nat_sessions: Dict[Tuple, NatSessionRec] = {}
        self.nat_reverse: Dict[Tuple, Tuple] = {}
        self.eim: Dict[Tuple, EimRec] = {}
        self.subnat: Dict[int, SubnatRec] = {}
        self.hairpin_ips: set = set()
        self.alg_ports: set = set()                   # (port, proto)
        self.nat_flags = abi.NAT_FLAG_EIM
        self.private_ranges: List[Tuple[int, int]] = list(DEFAULT_PRIVATE_RANGES)
        self.nat_stats = [0] * abi.NAT_NSTATS
        self.nat_log: List[dict] = []
        # QoS
        self.qos_egress: Dict[int, QosBucketRec] = {}
        self.qos_ingress: Dict[int, QosBucketRec] = {}
        self.qos_stats = [0] * abi.QOS_NSTATS
        # antispoof
        self.bindings: Dict[int, BindingRec] = {}
        self.as_default_mode = abi.AS_DISABLED
        self.as_log_violations = 0
        self.allowed_ranges: List[Tuple[int, int]] = []
        self.as_stats = [0] * abi.AS_NSTATS
        self.spoof_events: List[dict] = []
        # PPPoE session-data fast path
        self.pppoe_sessions: Dict[int, PppoeSessRec] = {}   # by session id
        self.pppoe_by_ip: Dict[int, Tuple[int, int]] = {}   # ip -> (sid, mac)
        self.pppoe_stats = [0] * abi.PPPOE_NSTATS
        # per-subscriber traffic accounting, by subscriber IPv4
        self.acct: Dict[int, AcctRec] = {}
        # walled-garden gate: subscriber IPv4 -> (mac as u64, abi.WG_*
        # state), and what a quarantined subscriber may reach
        self.wg: Dict[int, Tuple[int, int]] = {}
        self.wg_allowed: set = set()          # (ip, port, proto)
        self.wg_allowed_ips: set = set()      # the addresses of those keys
        self.wg_redirect_ports: set = set(abi.WG_DEFAULT_REDIRECT_PORTS)
        self.wg_stats = [0] * abi.WG_NSTATS

    # ------------------------------------------------------------- helpers
    @property
    def now_sec(self) -> int:
        return self.now_ns // 1_000_000_000

    def _is_private(self, ip: int) -> bool:
        for net, mask in self.private_ranges:
            if (ip & mask) == net:
                return True
        return False

    # =================================================== DHCP fast path K1
    def dhcp_fastpath(self, frame: bytearray) -> Tuple[int, int]:
        """Process one frame; returns (verdict, out_len).  On TX the frame
        is rewritten in place into the OFFER/ACK (ref dhcp_fastpath.c:619)."""
        n = len(frame)
        if n < 14:
            return PASS, n
        proto = struct.unpack_from(">H", frame, 12)[0]
        off = 14
        vlan_offset = 0
        s_tag = c_tag = 0
        tagged = False
        if proto in (ETH_P_8021Q, ETH_P_8021AD):
            if n < off + 4:
                return PASS, n
            tagged = True
            s_tag = struct.unpack_from(">H", frame, off)[0] & 0xFFF
            proto = struct.unpack_from(">H", frame, off + 2)[0]
            off += 4
            vlan_offset = 4
            self.dhcp_stats[abi.ST_VLAN_PACKETS] += 1
            if proto == ETH_P_8021Q:
                if n < off + 4:
                    return PASS, n
                c_tag = struct.unpack_from(">H", frame, off)[0] & 0xFFF
                proto = struct.unpack_from(">H", frame, off + 2)[0]
                off += 4
                vlan_offset = 8
        if proto != ETH_P_IP or n < off + 20:
            return PASS, n
        ip_off = off
        if not self._ipv4_header_ok(frame, ip_off):
            return PASS, n
        if frame[ip_off + 9] != 17:      # UDP
            return PASS, n
        if struct.unpack_from(">H", frame, ip_off + 6)[0] & 0x1FFF:
            return PASS, n               # non-first fragment: no UDP header
        ihl = (frame[ip_off] & 0xF) * 4
        udp_off = ip_off + ihl
        if n < udp_off + 8:
            return PASS, n
        dport = struct.unpack_from(">H", frame, udp_off + 2)[0]
        if dport != 67:
            return PASS, n
        dhcp_off = udp_off + 8
        if n < dhcp_off + 240:
            return PASS, n
        if frame[dhcp_off] != 1:         # BOOTREQUEST
            return PASS, n
        magic = struct.unpack_from(">I", frame, dhcp_off + 236)[0]
        if magic != 0x63825363:
            return PASS, n

        self.dhcp_stats[abi.ST_TOTAL_REQUESTS] += 1

        msg_type, circuit_id = self._scan_options(frame, dhcp_off + 240, n)
        if msg_type not in (1, 3):       # DISCOVER / REQUEST only
            self.dhcp_stats[abi.ST_FASTPATH_MISSES] += 1
            return PASS, n

        # 3-way lookup priority: VLAN -> circuit-ID -> MAC
        # (ref dhcp_fastpath.c:647-687)
        sub: Optional[SubRecord] = None
        if tagged:
            sub = self.subscribers.get(abi.vlan_key(s_tag, c_tag))
        if sub is None and circuit_id:
            sub = self.subscribers.get(abi.circuit_key(circuit_id))
            if sub is not None:
                self.dhcp_stats[abi.ST_OPTION82_PRESENT] += 1
        if sub is None:
            chaddr = bytes(frame[dhcp_off + 28:dhcp_off + 34])
            sub = self.subscribers.get(abi.mac_to_u64(chaddr))
        if sub is None:
            self.dhcp_stats[abi.ST_FASTPATH_MISSES] += 1
            return PASS, n
        if self.now_sec > sub.lease_expiry:
            self.dhcp_stats[abi.ST_CACHE_EXPIRED] += 1
            return PASS, n
        pool = self.pools.get(sub.pool_id)
        if pool is None:
            self.dhcp_stats[abi.ST_ERRORS] += 1
            return PASS, n
        self.dhcp_stats[abi.ST_FASTPATH_HITS] += 1

        reply_type = 2 if msg_type == 1 else 5   # OFFER : ACK
        giaddr = struct.unpack_from(">I", frame, dhcp_off + 24)[0]
        server_ip = self.server_ip if self.server_ip else pool.gateway

        if giaddr != 0:
            # relayed: unicast to relay agent (ref :726-743)
            frame[0:6] = frame[6:12]
            frame[6:12] = self.server_mac
            struct.pack_into(">I", frame, ip_off + 12, server_ip)
            struct.pack_into(">I", frame, ip_off + 16, giaddr)
            daddr_for_udp = giaddr
            struct.pack_into(">HH", frame, udp_off, 67, 67)
            self.dhcp_stats[abi.ST_UNICAST_REPLIES] += 1
        else:
            flags = struct.unpack_from(">H", frame, dhcp_off + 10)[0]
            ciaddr = struct.unpack_from(">I", frame, dhcp_off + 12)[0]
            chaddr = bytes(frame[dhcp_off + 28:dhcp_off + 34])
            use_broadcast = bool(flags & 0x8000) or ciaddr == 0
            if use_broadcast:
                frame[0:6] = b"\xff" * 6
                self.dhcp_stats[abi.ST_BROADCAST_REPLIES] += 1
            else:
                frame[0:6] = chaddr
                self.dhcp_stats[abi.ST_UNICAST_REPLIES] += 1
            frame[6:12] = self.server_mac
            struct.pack_into(">I", frame, ip_off + 12, server_ip)
            struct.pack_into(">I", frame, ip_off + 16, 0xFFFFFFFF)
            struct.pack_into(">HH", frame, udp_off, 67, 68)

        frame[ip_off + 8] = 64           # TTL
        struct.pack_into(">H", frame, udp_off + 6, 0)  # UDP csum 0

        # DHCP reply fixed fields (ref :759-766)
        frame[dhcp_off] = 2              # BOOTREPLY
        frame[dhcp_off + 3] = 0          # hops
        struct.pack_into(">I", frame, dhcp_off + 16, sub.allocated_ip)  # yiaddr
        struct.pack_into(">I", frame, dhcp_off + 20, server_ip)         # siaddr
        frame[dhcp_off + 44:dhcp_off + 236] = b"\x00" * 192  # sname+file

        # grow the buffer for the reply options if the request was shorter
        # (the XDP analog is bpf_xdp_adjust_tail, ref :799-809; the GPU path
        # has fixed-stride slots with headroom instead)
        need = dhcp_off + 240 + 64
        if len(frame) < need:
            frame.extend(b"\x00" * (need - len(frame)))
        opt_len = self._build_reply_options(
            frame, dhcp_off + 240, reply_type, pool, server_ip)

        dhcp_len = 240 + opt_len
        udp_len = 8 + dhcp_len
        ip_len = 20 + udp_len
        total = 14 + vlan_offset + ip_len
        struct.pack_into(">H", frame, ip_off + 2, ip_len)
        struct.pack_into(">H", frame, udp_off + 4, udp_len)
        struct.pack_into(">H", frame, ip_off + 10, 0)
        csum = ipv4_checksum(bytes(frame[ip_off:ip_off + 20]))
        struct.pack_into(">H", frame, ip_off + 10, csum)
        return TX, total

    @staticmethod
    def _scan_options(frame, opt_off: int, end: int) -> Tuple[int, bytes]:
        """Full TLV scan for option 53 and option-82 circuit-id.  Upgrade
        over the reference's fixed-offset scan (dhcp_fastpath.c:216-323);
        bounded like its MAX_DHCP_OPTIONS_ITER/SCAN_LEN (maps.h:19-22)."""
        msg_type = 0
        circuit_id = b""
        i = opt_off
        limit = min(end, opt_off + 312)
        iters = 0
        while i < limit and iters < 64:
            iters += 1
            code = frame[i]
            if code == 0:
                i += 1
                continue
            if code == 255:
                break
            if i + 1 >= limit:
                break
            ln = frame[i + 1]
            if i + 2 + ln > limit:
                break
            if code == 53 and ln == 1:
                msg_type = frame[i + 2]
            elif code == 82:
                j = i + 2
                sub_end = i + 2 + ln
                while j + 2 <= sub_end:
                    sc, sl = frame[j], frame[j + 1]
                    if j + 2 + sl > sub_end:
                        break
                    if sc == 1 and 0 < sl <= 32:
                        circuit_id = bytes(frame[j + 2:j + 2 + sl])
                    j += 2 + sl
            i += 2 + ln
        return msg_type, circuit_id

    @staticmethod
    def _build_reply_options(frame, off: int, reply_type: int,
                             pool: PoolRecord, server_ip: int) -> int:
        """Options 53/54/51/1/3/6/58/59/255 (ref build_dhcp_options :519-602)."""
        o = off
        frame[o:o + 3] = bytes([53, 1, reply_type]); o += 3
        frame[o:o + 2] = bytes([54, 4]); struct.pack_into(">I", frame, o + 2, server_ip); o += 6
        frame[o:o + 2] = bytes([51, 4]); struct.pack_into(">I", frame, o + 2, pool.lease_time); o += 6
        mask = 0 if pool.prefix_len == 0 else (0xFFFFFFFF << (32 - min(pool.prefix_len, 32))) & 0xFFFFFFFF
        frame[o:o + 2] = bytes([1, 4]); struct.pack_into(">I", frame, o + 2, mask); o += 6
        frame[o:o + 2] = bytes([3, 4]); struct.pack_into(">I", frame, o + 2, pool.gateway); o += 6
        if pool.dns_primary:
            dns_len = 8 if pool.dns_secondary else 4
            frame[o:o + 2] = bytes([6, dns_len])
            struct.pack_into(">I", frame, o + 2, pool.dns_primary)
            if pool.dns_secondary:
                struct.pack_into(">I", frame, o + 6, pool.dns_secondary)
            o += 2 + dns_len
        frame[o:o + 2] = bytes([58, 4]); struct.pack_into(">I", frame, o + 2, pool.lease_time // 2); o += 6
        frame[o:o + 2] = bytes([59, 4]); struct.pack_into(">I", frame, o + 2, (pool.lease_time * 7) // 8); o += 6
        frame[o] = 255; o += 1
        return o - off

    # ========================================================= NAT44 K2
    @staticmethod
    def _upd_csum(csum: int, old: int, new: int) -> int:
        """Incremental checksum for a 32-bit field (ref update_csum :384-391)."""
        s = (~csum) & 0xFFFF
        s += (~old & 0xFFFF) + ((~old >> 16) & 0xFFFF)
        s += (new & 0xFFFF) + (new >> 16)
        s = (s & 0xFFFF) + (s >> 16)
        s = (s & 0xFFFF) + (s >> 16)
        return (~s) & 0xFFFF

    @staticmethod
    def _upd_csum16(csum: int, old: int, new: int) -> int:
        s = (~csum) & 0xFFFF
        s += (~old & 0xFFFF) + (new & 0xFFFF)
        s = (s & 0xFFFF) + (s >> 16)
        s = (s & 0xFFFF) + (s >> 16)
        return (~s) & 0xFFFF

    def _alloc_port(self, blk: SubnatRec, preserve_parity: bool,
                    orig_port_host: int, internal_ip: int, proto: int) -> int:
        """RFC 6431 port rotor with EIM-collision check
        (ref allocate_port_from_block nat44.c:408-466)."""
        orig_parity = orig_port_host & 1
        for _ in range(64):
            port = blk.next_port & 0xFFFF
            blk.next_port += 1
            if port > blk.port_end:
                port = blk.port_start
            if blk.next_port > blk.port_end:
                blk.next_port = blk.port_start
            if preserve_parity and (port & 1) != orig_parity:
                continue
            if (internal_ip, port, proto) in self.eim:
                continue
            return port
        return 0

    @staticmethod
    def _ipv4_header_ok(frame, ip_off: int) -> bool:
        """Version 4 and ihl >= 5 (parse_pkt_slow).  The reference takes
        any header under ethertype 0x0800 (nat44.c:606); we do not: with
        ihl < 5 the "L4 header" lies inside the IP header and SNAT would
        write a port over it."""
        return frame[ip_off] >> 4 == 4 and (frame[ip_off] & 0xF) >= 5

    def _parse_l3l4(self, frame) -> Optional[dict]:
        """None: not IPv4.  `short`: the frame ends inside the TCP/UDP/ICMP
        header; the NAT stages forward it, but a private source without a
        NAT context is passed to the host first, as in the kernel.  `no_l4` is a TCP/UDP/ICMP packet without a flow identifier the fast
        path may use — a non-first fragment, whose L4 bytes are payload, or
        an ICMP message that is not a query and so has no id.  The reference
        reads ports and ids from both (nat44.c:606-648); we read and write
        none of their L4 bytes."""
        n = len(frame)
        if n < 34 or struct.unpack_from(">H", frame, 12)[0] != ETH_P_IP:
            return None
        ip_off = 14
        if not self._ipv4_header_ok(frame, ip_off):
            return None
        ihl = (frame[ip_off] & 0xF) * 4
        proto = frame[ip_off + 9]
        saddr, daddr = struct.unpack_from(">II", frame, ip_off + 12)
        l4 = ip_off + ihl
        r = dict(ip_off=ip_off, l4=l4, proto=proto, saddr=saddr, daddr=daddr,
                 no_l4=False, short=False)
        if struct.unpack_from(">H", frame, ip_off + 6)[0] & 0x1FFF:
            r["no_l4"] = proto in (6, 17, 1)
        elif proto == 6 and n >= l4 + 20:
            r["sport"], r["dport"] = struct.unpack_from(">HH", frame, l4)
            r["tcp_flags"] = frame[l4 + 13]
        elif proto == 17 and n >= l4 + 8:
            r["sport"], r["dport"] = struct.unpack_from(">HH", frame, l4)
        elif proto == 1 and n >= l4 + 8:
            if frame[l4] in ICMP_QUERY_TYPES:
                r["icmp_id"] = struct.unpack_from(">H", frame, l4 + 4)[0]
            else:
                r["no_l4"] = True
        elif proto in (6, 17, 1):
            r["short"] = True            # the frame ends inside the L4 header
        return r

    def nat44_egress(self, frame: bytearray) -> int:
        """SNAT (ref nat44_egress nat44.c:565-802).  Returns verdict.
        Unlike the reference, a non-first fragment or a non-query ICMP
        message from a NATed subscriber goes to the host (PASS), untouched."""
        h = self._parse_l3l4(frame)
        if h is None:
            return FWD
        if not self._is_private(h["saddr"]):
            return FWD
        blk = self.subnat.get(h["saddr"])
        if blk is None or h["no_l4"]:
            self.nat_stats[abi.NS_PASSED] += 1
            return PASS
        if h["short"]:
            return FWD
        proto = h["proto"]
        if proto == 6:
            sport, dport = h["sport"], h["dport"]
            if self.nat_flags & (abi.NAT_FLAG_ALG_FTP | abi.NAT_FLAG_ALG_SIP):
                if (dport, 6) in self.alg_ports:
                    self.nat_stats[abi.NS_ALG_TRIGGERS] += 1
                    self._log(abi.LOG_ALG_TRIGGER, blk.subscriber_id,
                              h["saddr"], 0, sport, 0, h["daddr"], dport, 6)
                    return PASS
        elif proto == 17:
            sport, dport = h["sport"], h["dport"]
            if self.nat_flags & abi.NAT_FLAG_ALG_SIP:
                if (dport, 17) in self.alg_ports:
                    self.nat_stats[abi.NS_ALG_TRIGGERS] += 1
                    self._log(abi.LOG_ALG_TRIGGER, blk.subscriber_id,
                              h["saddr"], 0, sport, 0, h["daddr"], dport, 17)
                    return PASS
        elif proto == 1:
            sport, dport = h["icmp_id"], 0
        else:
            return FWD

        is_hairpin = 0
        if (self.nat_flags & abi.NAT_FLAG_HAIRPIN) and h["daddr"] in self.hairpin_ips:
            is_hairpin = 1
            self.nat_stats[abi.NS_HAIRPIN] += 1

        key = (h["saddr"], h["daddr"], sport, dport, proto)
        sess = self.nat_sessions.get(key)
        now = self.now_ns
        if sess is not None:
            nat_ip, nat_port = sess.nat_ip, sess.nat_port
            sess.last_seen = now
            sess.packets_out += 1
            sess.bytes_out += len(frame)
        else:
            nat_ip = nat_port = None
            if self.nat_flags & abi.NAT_FLAG_EIM:
                ek = (h["saddr"], sport, proto)
                eim = self.eim.get(ek)
                if eim is not None:
                    eim.last_used = now
                    eim.ref_count += 1
                    self.nat_stats[abi.NS_EIM_HITS] += 1
                    nat_ip, nat_port = eim.external_ip, eim.external_port
                else:
                    p = self._alloc_port(blk, bool(self.nat_flags & abi.NAT_FLAG_PARITY),
                                         sport, h["saddr"], proto)
                    if p == 0:
                        self.nat_stats[abi.NS_PORT_EXHAUSTION] += 1
                        self.nat_stats[abi.NS_DROPPED] += 1
                        self._log(abi.LOG_PORT_EXHAUSTION, blk.subscriber_id,
                                  h["saddr"], blk.public_ip, sport, 0,
                                  h["daddr"], dport, proto)
                        return DROP
                    self.eim[ek] = EimRec(blk.public_ip, p, now, now, 1)
                    self.nat_stats[abi.NS_EIM_MISSES] += 1
                    nat_ip, nat_port = blk.public_ip, p
            if nat_ip is None:
                p = self._alloc_port(blk, bool(self.nat_flags & abi.NAT_FLAG_PARITY),
                                     sport, h["saddr"], proto)
                if p == 0:
                    self.nat_stats[abi.NS_PORT_EXHAUSTION] += 1
                    self.nat_stats[abi.NS_DROPPED] += 1
                    self._log(abi.LOG_PORT_EXHAUSTION, blk.subscriber_id,
                              h["saddr"], blk.public_ip, sport, 0,
                              h["daddr"], dport, proto)
                    return DROP
                nat_ip, nat_port = blk.public_ip, p
            sess = NatSessionRec(nat_ip, nat_port, sport, h["saddr"],
                                 h["daddr"], dport, abi.NAT_NEW, is_hairpin,
                                 now, now, 1, 0, len(frame), 0, proto)
            self.nat_sessions[key] = sess
            rev = (h["daddr"], nat_ip, dport, nat_port, proto)
            self.nat_reverse[rev] = key
            blk.sessions_active += 1
            blk.sessions_total += 1
            self.nat_stats[abi.NS_SESS_CREATED] += 1
            self._log(abi.LOG_SESSION_CREATE, blk.subscriber_id, h["saddr"],
                      nat_ip, sport, nat_port, h["daddr"], dport, proto,
                      is_hairpin)

        # rewrite (ref :752-798)
        ip_off, l4 = h["ip_off"], h["l4"]
        old_ip = h["saddr"]
        struct.pack_into(">I", frame, ip_off + 12, nat_ip)
        ipck = struct.unpack_from(">H", frame, ip_off + 10)[0]
        struct.pack_into(">H", frame, ip_off + 10,
                         self._upd_csum(ipck, old_ip, nat_ip))
        if proto == 6:
            old_port = struct.unpack_from(">H", frame, l4)[0]
            struct.pack_into(">H", frame, l4, nat_port)
            ck = struct.unpack_from(">H", frame, l4 + 16)[0]
            ck = self._upd_csum(ck, old_ip, nat_ip)
            ck = self._upd_csum16(ck, old_port, nat_port)
            struct.pack_into(">H", frame, l4 + 16, ck)
        elif proto == 17:
            old_port = struct.unpack_from(">H", frame, l4)[0]
            struct.pack_into(">H", frame, l4, nat_port)
            ck = struct.unpack_from(">H", frame, l4 + 6)[0]
            if ck != 0:
                ck = self._upd_csum(ck, old_ip, nat_ip)
                ck = self._upd_csum16(ck, old_port, nat_port)
                if ck == 0:
                    ck = 0xFFFF
                struct.pack_into(">H", frame, l4 + 6, ck)
        elif proto == 1:
            old_id = struct.unpack_from(">H", frame, l4 + 4)[0]
            struct.pack_into(">H", frame, l4 + 4, nat_port)
            ck = struct.unpack_from(">H", frame, l4 + 2)[0]
            struct.pack_into(">H", frame, l4 + 2,
                             self._upd_csum16(ck, old_id, nat_port))
        self.nat_stats[abi.NS_SNAT] += 1
        return FWD

    def nat44_ingress(self, frame: bytearray) -> int:
        """DNAT (ref nat44_ingress nat44.c:805-948).  Unlike the reference,
        non-first fragments and non-query ICMP are forwarded unread."""
        h = self._parse_l3l4(frame)
        if h is None:
            return FWD
        if h["no_l4"] or h["short"]:
            if h["proto"] == 1 and self.nat_flags & abi.NAT_FLAG_ICMP_ERR:
                self._nat44_ingress_icmp_error(frame, h)
            return FWD
        proto = h["proto"]
        if proto == 6 or proto == 17:
            sport, dport = h["sport"], h["dport"]
        elif proto == 1:
            sport, dport = 0, h["icmp_id"]
        else:
            return FWD
        rev = (h["saddr"], h["daddr"], sport, dport, proto)
        orig_key = self.nat_reverse.get(rev)
        if orig_key is None:
            self.nat_stats[abi.NS_PASSED] += 1
            return FWD
        sess = self.nat_sessions.get(orig_key)
        if sess is None:
            del self.nat_reverse[rev]
            self.nat_stats[abi.NS_SESS_EXPIRED] += 1
            return FWD
        sess.last_seen = self.now_ns
        sess.packets_in += 1
        sess.bytes_in += len(frame)
        if proto == 6:
            fl = h["tcp_flags"]
            if fl & 0x05:                       # FIN|RST
                sess.state = abi.NAT_CLOSING
            elif sess.state == abi.NAT_NEW and fl & 0x10:  # ACK
                sess.state = abi.NAT_ESTABLISHED

        ip_off, l4 = h["ip_off"], h["l4"]
        old_ip, new_ip = h["daddr"], sess.orig_ip
        struct.pack_into(">I", frame, ip_off + 16, new_ip)
        ipck = struct.unpack_from(">H", frame, ip_off + 10)[0]
        struct.pack_into(">H", frame, ip_off + 10,
                         self._upd_csum(ipck, old_ip, new_ip))
        new_port = sess.orig_port
        if proto == 6:
            old_port = struct.unpack_from(">H", frame, l4 + 2)[0]
            struct.pack_into(">H", frame, l4 + 2, new_port)
            ck = struct.unpack_from(">H", frame, l4 + 16)[0]
            ck = self._upd_csum(ck, old_ip, new_ip)
            ck = self._upd_csum16(ck, old_port, new_port)
            struct.pack_into(">H", frame, l4 + 16, ck)
        elif proto == 17:
            old_port = struct.unpack_from(">H", frame, l4 + 2)[0]
            struct.pack_into(">H", frame, l4 + 2, new_port)
            ck = struct.unpack_from(">H", frame, l4 + 6)[0]
            if ck != 0:
                ck = self._upd_csum(ck, old_ip, new_ip)
                ck = self._upd_csum16(ck, old_port, new_port)
                if ck == 0:
                    ck = 0xFFFF
                struct.pack_into(">H", frame, l4 + 6, ck)
        elif proto == 1:
            old_id = struct.unpack_from(">H", frame, l4 + 4)[0]
            struct.pack_into(">H", frame, l4 + 4, new_port)
            ck = struct.unpack_from(">H", frame, l4 + 2)[0]
            struct.pack_into(">H", frame, l4 + 2,
                             self._upd_csum16(ck, old_id, new_port))
        self.nat_stats[abi.NS_DNAT] += 1
        return FWD

    def _nat44_ingress_icmp_error(self, frame: bytearray, h: dict) -> None:
        """An inbound ICMP message DNAT forwards unread, under
        NAT_FLAG_ICMP_ERR (RFC 5508 REQ-3/4/5; nat_ingress_icmp_error in
        the kernels).  A Destination Unreachable, Time Exceeded or Parameter
        Problem whose quoted datagram is a flow of ours gets the outer
        destination and the quoted source address and port (or query id)
        set back to the subscriber's, every checksum over a changed word
        updated incrementally.  Reads the tables and writes none of them:
        no last_seen, no counters or state of the session, no cleaning of a
        stale reverse entry.  The verdict is FWD whatever happens here."""
        n, ip_off, l4 = len(frame), h["ip_off"], h["l4"]
        u16 = lambda o: struct.unpack_from(">H", frame, o)[0]
        if u16(ip_off + 6) & 0x1FFF or n < l4 + 8 or \
                frame[l4] not in (3, 11, 12):
            return                     # as with the flag off: not counted
        hit = self._icmp_error_flow(frame, h["daddr"], l4 + 8)
        if hit is None:
            self.nat_stats[abi.NS_ICMP_ERR_NOMAP] += 1
            return
        e, q, proto, id_at, pub_ip, pub_port, sess = hit
        new_ip, new_port = sess.orig_ip, sess.orig_port
        put16 = lambda o, v: struct.pack_into(">H", frame, o, v)
        # 1. outer destination and header checksum
        struct.pack_into(">I", frame, ip_off + 16, new_ip)
        put16(ip_off + 10, self._upd_csum(u16(ip_off + 10), pub_ip, new_ip))
        ock = u16(l4 + 2)              # follows every quoted word that changes
        # 2. quoted source and header checksum
        struct.pack_into(">I", frame, e + 12, new_ip)
        ock = self._upd_csum(ock, pub_ip, new_ip)
        ck = u16(e + 10)
        nk = self._upd_csum(ck, pub_ip, new_ip)
        put16(e + 10, nk)
        ock = self._upd_csum16(ock, ck, nk)
        # 3. quoted source port or id
        put16(id_at, new_port)
        ock = self._upd_csum16(ock, pub_port, new_port)
        # 4. quoted L4 checksum, where the quote reaches it
        ck_at = q + {6: 16, 17: 6, 1: 2}[proto]
        if n >= ck_at + 2:
            ck = nk = u16(ck_at)
            if proto == 1:
                nk = self._upd_csum16(ck, pub_port, new_port)
            elif proto == 6 or ck != 0:
                nk = self._upd_csum(ck, pub_ip, new_ip)
                nk = self._upd_csum16(nk, pub_port, new_port)
                if proto == 17 and nk == 0:
                    nk = 0xFFFF
            if nk != ck:
                put16(ck_at, nk)
                ock = self._upd_csum16(ock, ck, nk)
        # 5. outer ICMP checksum
        put16(l4 + 2, ock)
        self.nat_stats[abi.NS_ICMP_ERR_XLATE] += 1

    def _icmp_error_flow(self, frame, outer_daddr: int, e: int):
        """The session the datagram quoted at `e` belongs to, or None:
        (e, quoted L4 offset, protocol, offset of the public port or id,
        public ip, public port or id, session)."""
        n = len(frame)
        if n < e + 20 or not self._ipv4_header_ok(frame, e):
            return None
        q = e + (frame[e] & 0xF) * 4
        if n < q + 8 or struct.unpack_from(">H", frame, e + 6)[0] & 0x1FFF:
            return None
        pub_ip, remote_ip = struct.unpack_from(">II", frame, e + 12)
        if pub_ip != outer_daddr:
            return None
        proto = frame[e + 9]
        if proto in (6, 17):
            id_at, sport = q, struct.unpack_from(">H", frame, q + 2)[0]
        elif proto == 1 and frame[q] in ICMP_QUERY_TYPES:
            id_at, sport = q + 4, 0
        else:
            return None
        pub_port = struct.unpack_from(">H", frame, id_at)[0]
        orig_key = self.nat_reverse.get(
            (remote_ip, pub_ip, sport, pub_port, proto))
        sess = self.nat_sessions.get(orig_key) if orig_key else None
        if sess is None:
            return None
        return e, q, proto, id_at, pub_ip, pub_port, sess

    def _log(self, ev, sub_id, priv_ip, pub_ip, priv_port, pub_port,
             dest_ip, dest_port, proto, flags=0):
        self.nat_log.append(dict(
            timestamp=self.now_ns, event_type=ev, subscriber_id=sub_id,
            private_ip=priv_ip, public_ip=pub_ip, private_port=priv_port,
            public_port=pub_port, dest_ip=dest_ip, dest_port=dest_port,
            protocol=proto, flags=flags))

    # =========================================================== QoS K3
    def _tb_check(self, tb: QosBucketRec, pkt_len: int) -> bool:
        """Token bucket (ref token_bucket_check qos_ratelimit.c:70-104).
        Unlike the reference, a clock that has not moved past last_update
        (a wall clock stepped back) earns nothing and leaves the stamp
        alone, as on the device; the reference would subtract tokens."""
        if tb.rate_bps == 0:
            return True
        elapsed = self.now_ns - tb.last_update
        if elapsed > 0:
            tb.tokens += (elapsed * (tb.rate_bps // 8)) // 1_000_000_000
            if tb.tokens > tb.burst_bytes:
                tb.tokens = tb.burst_bytes
            tb.last_update = self.now_ns
        if tb.tokens >= pkt_len:
            tb.tokens -= pkt_len
            return True
        return False

    def qos(self, frame: bytes, direction: str) -> int:
        """direction 'egress' keys dst IP (download), 'ingress' src IP."""
        if len(frame) < 34 or struct.unpack_from(">H", frame, 12)[0] != ETH_P_IP:
            return FWD
        if not self._ipv4_header_ok(frame, 14):
            return FWD
        saddr, daddr = struct.unpack_from(">II", frame, 14 + 12)
        table =self.qos_egress if direction == "egress" else self.qos_ingress
        tb = table.get(daddr if direction == "egress" else saddr)
        if tb is None:
            return FWD
        allowed = self._tb_check(tb, len(frame))
        if allowed:
            self.qos_stats[abi.QS_PKT_PASSED] += 1
            self.qos_stats[abi.QS_BYTES_PASSED] += len(frame)
            return FWD
        self.qos_stats[abi.QS_PKT_DROPPED] += 1
        self.qos_stats[abi.QS_BYTES_DROPPED] += len(frame)
        return DROP

    # ============================================== PPPoE session data
    def pppoe_add_session(self, session_id: int, client_mac, ip: int,
                          mru: int = 1492):
        """Upsert; re-using a session id with another address removes the
        stale by-IP entry (pppoe_sess_upsert_kernel)."""
        sid = session_id & 0xFFFF
        mac = client_mac if isinstance(client_mac, int) \
            else abi.mac_to_u64(bytes(client_mac))
        old = self.pppoe_sessions.get(sid)
        if old is not None and old.ip != ip and \
                self.pppoe_by_ip.get(old.ip, (None,))[0] == sid:
            del self.pppoe_by_ip[old.ip]
        self.pppoe_sessions[sid] = PppoeSessRec(mac, ip, mru)
        self.pppoe_by_ip[ip] = (sid, mac)

    def pppoe_remove_session(self, session_id: int):
        sid = session_id & 0xFFFF
        old = self.pppoe_sessions.pop(sid, None)
        # only the owner removes the by-IP entry: the address may already
        # belong to a newer session
        if old is not None and \
                self.pppoe_by_ip.get(old.ip, (None,))[0] == sid:
            del self.pppoe_by_ip[old.ip]

    def pppoe_decap(self, frame: bytearray) -> Tuple[int, int]:
        """Uplink pre-pass (pppoe_decap_kernel): a 0x8864 frame carrying
        PPP IPv4 from a provisioned session is rewritten in place into the
        untagged IPoE frame with the same IP packet.  Returns (state,
        new_len); bytes at and beyond new_len are unspecified."""
        n = len(frame)
        if n < 14 or struct.unpack_from(">H", frame, 12)[0] != 0x8864:
            return abi.PPPOE_NONE, n
        st = self.pppoe_stats
        if n < 22:
            st[abi.PS_DECAP_MALFORMED] += 1
            return abi.PPPOE_REJECT, n
        if frame[14] != 0x11 or frame[15] != 0x00:
            st[abi.PS_DECAP_MALFORMED] += 1
            return abi.PPPOE_REJECT, n
        plen = struct.unpack_from(">H", frame, 18)[0]
        if plen < 2 or 20 + plen > n:
            st[abi.PS_DECAP_MALFORMED] += 1
            return abi.PPPOE_REJECT, n
        if struct.unpack_from(">H", frame, 20)[0] != 0x0021:
            # LCP / auth / IPCP / IPv6: the host PPPoE server's business;
            # checked before the session lookup because the table holds a
            # session only from IPCP-open
            st[abi.PS_DECAP_CTRL] += 1
            return abi.PPPOE_CTRL, n
        sess = self.pppoe_sessions.get(struct.unpack_from(">H", frame, 16)[0])
        if sess is None:
            st[abi.PS_DECAP_UNKNOWN_SESSION] += 1
            return abi.PPPOE_REJECT, n
        if abi.mac_to_u64(bytes(frame[6:12])) != sess.mac:
            st[abi.PS_DECAP_MAC_MISMATCH] += 1
            return abi.PPPOE_REJECT, n
        if plen - 2 < 20:
            st[abi.PS_DECAP_MALFORMED] += 1
            return abi.PPPOE_REJECT, n
        frame[12:14] = b"\x08\x00"
        frame[14:12 + plen] = frame[22:20 + plen]
        st[abi.PS_DECAP_OK] += 1
        return abi.PPPOE_DECAP, 12 + plen      # Ethernet padding trimmed

    def pppoe_encap(self, frame: bytearray, verdict: int,
                    stride: int) -> Tuple[int, int, int]:
        """Downlink post-pass (pppoe_encap_kernel): a forwarded IPv4 frame
        whose (DNAT-ed) destination is a PPPoE subscriber gets the session
        header back, in place (the bytearray grows by 8).  Returns (state,
        verdict, new_len)."""
        n = len(frame)
        if verdict != FWD or n < 34 or \
                struct.unpack_from(">H", frame, 12)[0] != ETH_P_IP:
            return abi.PPPOE_NONE, verdict, n
        hit = self.pppoe_by_ip.get(struct.unpack_from(">I", frame, 30)[0])
        sess = self.pppoe_sessions.get(hit[0]) if hit is not None else None
        if sess is None:
            return abi.PPPOE_NONE, verdict, n
        sid, mac = hit
        if n - 14 > sess.mru:
            # the host decides between fragmentation and ICMP
            self.pppoe_stats[abi.PS_ENCAP_TOO_BIG] += 1
            return abi.PPPOE_TOO_BIG, PASS, n
        if n + 8 > stride:
            self.pppoe_stats[abi.PS_ENCAP_NO_ROOM] += 1
            return abi.PPPOE_NO_ROOM, PASS, n
        frame[0:14] = (mac.to_bytes(6, "big") + bytes(self.server_mac) +
                       b"\x88\x64" +
                       struct.pack(">BBHHH", 0x11, 0x00, sid, n - 14 + 2,
                                   0x0021))
        self.pppoe_stats[abi.PS_ENCAP_OK] += 1
        return abi.PPPOE_ENCAP, verdict, n + 8

    # ===================================== per-subscriber accounting
    def acct_resolve(self, frame, by: str = "src") -> Optional[int]:
        """The accounted address of an untagged IPv4 frame — its source
        (uplink, BEFORE the pipeline: SNAT overwrites it) or destination
        (downlink, AFTER the pipeline: DNAT has restored it) — or None:
        not untagged IPv4, too short, or nobody accounts that address
        (acct_resolve_kernel / acct_downlink_kernel)."""
        if len(frame) < 34 or \
                struct.unpack_from(">H", frame, 12)[0] != ETH_P_IP:
            return None
        ip = struct.unpack_from(">I", frame, 26 if by == "src" else 30)[0]
        return ip if ip in self.acct else None

    def acct_commit(self, key: Optional[int], direction: str, length: int,
                    verdict: int, now_ns: int):
        """Bill one packet to acct_resolve's key: FWD adds (1, length) and
        stamps last_seen, DROP adds one dropped packet, PASS and TX count
        nothing (acct_commit_kernel)."""
        e = self.acct.get(key) if key is not None else None
        if e is None:
            return
        up = direction == "uplink"
        if verdict == FWD:
            if up:
                e.up_pkts += 1
                e.up_bytes += length
            else:
                e.down_pkts += 1
                e.down_bytes += length
            e.last_seen = now_ns
        elif verdict == DROP:
            if up:
                e.up_drop_pkts += 1
            else:
                e.down_drop_pkts += 1

    # ================================================ walled-garden gate
    def wg_set_config(self, allowed, redirect_ports=None):
        """The allow-list as (ip, port, proto) ints and the TCP ports whose
        traffic goes to the host for the portal redirect."""
        keys, ips, ports = abi.wg_fold_config(
            allowed, abi.WG_DEFAULT_REDIRECT_PORTS
            if redirect_ports is None else redirect_ports)
        self.wg_allowed = {(k >> 32, (k >> 16) & 0xFFFF, k & 0xFF)
                           for k in keys}
        self.wg_allowed_ips = set(ips)
        self.wg_redirect_ports = set(ports)

    def _garden_parse(self, frame) -> Optional[dict]:
        """None: the gate does not judge this frame (shorter than 34 B,
        tagged or not IPv4, version != 4, ihl < 5).  `ports`: TCP or UDP,
        first fragment, and the frame holds the whole TCP (20 B) / UDP
        (8 B) header, wherever IP options put it; every other frame is
        portless (another protocol, ICMP included, a non-first fragment, a
        truncated L4 header)."""
        n = len(frame)
        if n < 34 or struct.unpack_from(">H", frame, 12)[0] != ETH_P_IP:
            return None
        if not self._ipv4_header_ok(frame, 14):
            return None
        proto = frame[23]
        saddr, daddr = struct.unpack_from(">II", frame, 26)
        l4 = 14 + (frame[14] & 0xF) * 4
        r = dict(saddr=saddr, daddr=daddr, proto=proto, ports=False,
                 sport=0, dport=0, smac=abi.mac_to_u64(bytes(frame[6:12])))
        frag = struct.unpack_from(">H", frame, 20)[0] & 0x1FFF
        if proto in (6, 17) and not frag and \
                n >= l4 + (20 if proto == 6 else 8):
            r["sport"], r["dport"] = struct.unpack_from(">HH", frame, l4)
            r["ports"] = True
        return r

    def _garden_allowed(self, h: dict, ip: int, port: int) -> bool:
        if h["ports"]:
            return (ip, port, h["proto"]) in self.wg_allowed
        return ip in self.wg_allowed_ips

    def garden_uplink(self, frame) -> Tuple[int, Optional[int]]:
        """The uplink gate's decision for one frame, keyed on its source
        address (wg_uplink_kernel): (gate code, verdict).  Gate NONE has
        verdict None — the pipeline decides, as without a garden; every
        other gate fixes the verdict, the frame keeps its bytes and length
        and never enters the pipeline.  In table order:

          not judged, or source not in the garden      NONE
          entry BLOCKED                                DROP_BLOCKED  DROP
          WALLED, source MAC is not the entry's        DROP_MAC      DROP
          WALLED, UDP to port 67 (a lease renewal)     NONE
          WALLED, (daddr, dport, proto) allow-listed   ALLOW         FWD
          WALLED, TCP to a redirect port               REDIRECT      PASS
          WALLED, portless, daddr allow-listed         ALLOW         FWD
          WALLED, anything else                        DROP_WALLED   DROP

        ALLOW forwards without NAT: the portal and its resolvers sit inside
        the operator's network.  The last four rows are Manager.classify()
        with port 0 for a portless frame; a frame with readable ports to
        port 0 is the one place they differ (classify takes port 0 as "no
        port", the gate looks (daddr, 0, proto) up and drops)."""
        h = self._garden_parse(frame)
        e = self.wg.get(h["saddr"]) if h is not None else None
        if e is None:
            return abi.WG_NONE, None
        mac, state = e
        st = self.wg_stats
        if state == abi.WG_BLOCKED:
            st[abi.WS_UP_DROP_BLOCKED] += 1
            return abi.WG_DROP_BLOCKED, DROP
        if state != abi.WG_WALLED:
            return abi.WG_NONE, None
        if h["smac"] != mac:
            st[abi.WS_UP_DROP_MAC] += 1
            return abi.WG_DROP_MAC, DROP
        if h["ports"] and h["proto"] == 17 and h["dport"] == 67:
            return abi.WG_NONE, None
        if self._garden_allowed(h, h["daddr"], h["dport"]):
            st[abi.WS_UP_ALLOWED] += 1
            return abi.WG_ALLOW, FWD
        if h["ports"] and h["proto"] == 6 and \
                h["dport"] in self.wg_redirect_ports:
            st[abi.WS_UP_REDIRECTED] += 1
            return abi.WG_REDIRECT, PASS
        st[abi.WS_UP_DROP_WALLED] += 1
        return abi.WG_DROP_WALLED, DROP

    def garden_downlink(self, frame, verdict: int) -> Tuple[int, int]:
        """The downlink gate (wg_downlink_kernel), after the pipeline: a
        forwarded frame whose DNAT-rewritten destination is in the garden
        stays FWD only if the entry is WALLED and its source is
        allow-listed — (saddr, sport, proto), or the bare address for a
        portless frame.  Returns (gate code, verdict); the gate can only
        turn FWD into DROP."""
        if verdict != FWD:
            return abi.WG_NONE, verdict
        h = self._garden_parse(frame)
        e = self.wg.get(h["daddr"]) if h is not None else None
        if e is None:
            return abi.WG_NONE, verdict
        _mac, state = e
        st = self.wg_stats
        if state == abi.WG_BLOCKED:
            st[abi.WS_DOWN_DROP_BLOCKED] += 1
            return abi.WG_DROP_BLOCKED, DROP
        if state != abi.WG_WALLED:
            return abi.WG_NONE, verdict
        if self._garden_allowed(h, h["saddr"], h["sport"]):
            st[abi.WS_DOWN_ALLOWED] += 1
            return abi.WG_ALLOW, FWD
        st[abi.WS_DOWN_DROP_WALLED] += 1
        return abi.WG_DROP_WALLED, DROP

    # ====================================================== antispoof K4
    def antispoof(self, frame: bytes) -> int:
        """uRPF source validation (ref antispoof_ingress antispoof.c:189-293).
        The reference's binding+LOOSE fallthrough quirk (a valid binding in
        LOOSE mode is never range-checked and always violates, :227-235) is
        preserved for behavioral parity."""
        if len(frame) < 14:
            return FWD
        mac = abi.mac_to_u64(bytes(frame[6:12]))
        b = self.bindings.get(mac)
        mode = b.mode if b is not None else self.as_default_mode
        if mode == abi.AS_DISABLED:
            self.as_stats[abi.AS_ALLOWED] += 1
            return FWD
        proto = struct.unpack_from(">H", frame, 12)[0]
        if proto == ETH_P_IP:
            if len(frame) < 34:
                return FWD
            src_ip = struct.unpack_from(">I", frame, 14 + 12)[0]
            allowed = False
            if b is not None and b.ipv4_valid:
                if mode in (abi.AS_STRICT, abi.AS_LOG_ONLY):
                    allowed = src_ip == b.ipv4_addr
            elif mode == abi.AS_LOOSE:
                allowed = any((src_ip & m) == net
                              for net, m in self.allowed_ranges)
            if not allowed:
                if self.as_log_violations:
                    self.spoof_events.append(dict(
                        timestamp=self.now_ns, src_mac=bytes(frame[6:12]),
                        protocol=4, spoofed_ip=src_ip,
                        allowed_ip=b.ipv4_addr if b else 0))
                    self.as_stats[abi.AS_LOGGED] += 1
                if mode == abi.AS_LOG_ONLY:
                    self.as_stats[abi.AS_ALLOWED] += 1
                    return FWD
                self.as_stats[abi.AS_DROPPED] += 1
                self.as_stats[abi.AS_V4_VIOLATIONS] += 1
                return DROP
            self.as_stats[abi.AS_ALLOWED] += 1
            return FWD
        if proto == ETH_P_IPV6:
            if len(frame) < 14 + 40:
                return FWD
            src6 = bytes(frame[14 + 8:14 + 24])
            allowed = False
            if b is not None and b.ipv6_valid:
                allowed = src6 == b.ipv6_addr
            elif mode == abi.AS_LOOSE:
                allowed = True
            if not allowed and mode != abi.AS_LOG_ONLY:
                if self.as_log_violations:
                    self.spoof_events.append(dict(
                        timestamp=self.now_ns, src_mac=bytes(frame[6:12]),
                        protocol=6, spoofed_ip=0, allowed_ip=0))
                    self.as_stats[abi.AS_LOGGED] += 1
                self.as_stats[abi.AS_DROPPED] += 1
                self.as_stats[abi.AS_V6_VIOLATIONS] += 1
                return DROP
            self.as_stats[abi.AS_ALLOWED] += 1
            return FWD
        self.as_stats[abi.AS_ALLOWED] += 1
        return FWD
