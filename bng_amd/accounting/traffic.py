"""Feeds the dataplane's per-subscriber counters to RADIUS accounting.

A lease's address is accounted on the device from the moment the lease
exists (launcher.acct_add) until it is torn down (launcher.acct_remove,
which returns the final counters in the same stream-ordered step).
AccountingManager pulls the numbers through fetch() before every
Interim-Update and Stop record (ref pkg/radius/accounting.go
SetCounterFetcher).

Works over HipLauncher and GoldenLauncher alike."""
from __future__ import annotations

import socket
import struct
import threading
from typing import Dict, Optional, Tuple


def _ip_to_u32(ip) -> int:
    if isinstance(ip, int):
        return ip & 0xFFFFFFFF
    return struct.unpack(">I", socket.inet_aton(ip))[0]


def _counters(row) -> Tuple[int, int, int, int]:
    """(input_octets, output_octets, input_packets, output_packets): RFC
    2866 input is what the NAS received from the subscriber's port."""
    return (int(row["up_bytes"]), int(row["down_bytes"]),
            int(row["up_pkts"]), int(row["down_pkts"]))


class TrafficAccounting:
    def __init__(self, launcher, max_parked: int = 65536):
        self.launcher = launcher
        self.max_parked = max_parked
        # final counters of torn-down leases, by address, until the Stop
        # record picks them up: DHCPServer._teardown emits "delete" before
        # it calls accounting.stop_session
        self._final: Dict[int, Tuple[int, int, int, int]] = {}
        self._lock = threading.Lock()

    def on_lease_event(self, event: str, lease):
        """DHCPServer.on_lease_event listener."""
        ip = _ip_to_u32(lease.ip)
        if event == "add":
            with self._lock:
                self._final.pop(ip, None)   # the address has a new owner
            self.launcher.acct_add([ip])
        elif event == "delete":
            rows = self.launcher.acct_remove([ip])
            if len(rows) and int(rows[0]["key"]):
                with self._lock:
                    if len(self._final) >= self.max_parked:
                        # a Stop record that never came: drop the oldest
                        self._final.pop(next(iter(self._final)))
                    self._final[ip] = _counters(rows[0])

    def fetch(self, rec) -> Optional[Tuple[int, int, int, int]]:
        """AccountingManager counter fetcher: a parked final (popped) before
        a live read; None keeps the record's pushed values."""
        if not getattr(rec, "framed_ip", ""):
            return None
        ip = _ip_to_u32(rec.framed_ip)
        with self._lock:
            final = self._final.pop(ip, None)
        if final is not None:
            return final
        rows = self.launcher.acct_read([ip])
        if not len(rows) or not int(rows[0]["key"]):
            return None
        return _counters(rows[0])
