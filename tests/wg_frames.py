"""Frame builders and constants shared by the walled-garden gate tests
(test_walledgarden_dataplane.py on the golden model, test_walledgarden_gpu.py
on the device).  Plain byte assembly: the gate reads headers only, so L4
checksums are left zero."""
import struct

from bng_amd.dataplane import abi
from bng_amd.dataplane.packets import ip2u32

SERVER_MAC = bytes.fromhex("020000000001")
CORE_MAC = bytes.fromhex("020000000002")
PORTAL = ip2u32("10.255.255.1")
PORTAL_PORT = 8443
DNS = ip2u32("10.255.255.53")
OTHER = ip2u32("93.184.216.34")

# the garden Manager(portal, [dns], portal_port=PORTAL_PORT) builds
ALLOWED = [(DNS, 53, 17), (DNS, 53, 6), (PORTAL, PORTAL_PORT, 6)]


def raw_ipv4(smac, dmac, src, dst, proto, sport=0, dport=0, *, ihl=5,
             frag=0, l4_len=None, payload=0, version=4):
    """Ethernet + IPv4 (+ 4*(ihl-5) option bytes) + an L4 header of
    `l4_len` bytes (default: the protocol's full header: TCP 20, UDP 8,
    anything else 8) + `payload` zero bytes.  `l4_len` short of the full
    header truncates the frame inside it."""
    full = 20 if proto == 6 else 8
    if proto == 6:
        l4 = struct.pack(">HHIIBBHHH", sport, dport, 1, 1, 0x50, 0x10,
                         8192, 0, 0)
    elif proto == 17:
        l4 = struct.pack(">HHHH", sport, dport, 8 + payload, 0)
    else:
        l4 = struct.pack(">BBHHH", 8, 0, 0, sport, 1)
    l4 = l4[:full if l4_len is None else l4_len]
    body = l4 + bytes(payload)
    total = 4 * ihl + len(body)
    ip = struct.pack(">BBHHHBBHII", (version << 4) | ihl, 0, total, 0, frag,
                     64, proto, 0, src, dst) + bytes(4 * (ihl - 5))
    return bytes(dmac) + bytes(smac) + b"\x08\x00" + ip + body


def vlan_tagged(frame, vid=100):
    return frame[:12] + b"\x81\x00" + struct.pack(">H", vid) + frame[12:]


def arp_from(smac):
    return SERVER_MAC + bytes(smac) + b"\x08\x06" + bytes(28)


GATE_NAMES = {abi.WG_NONE: "NONE", abi.WG_ALLOW: "ALLOW",
              abi.WG_REDIRECT: "REDIRECT",
              abi.WG_DROP_WALLED: "DROP_WALLED",
              abi.WG_DROP_BLOCKED: "DROP_BLOCKED",
              abi.WG_DROP_MAC: "DROP_MAC"}
