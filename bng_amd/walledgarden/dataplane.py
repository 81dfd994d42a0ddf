"""Walled-garden enforcement on the dataplane: keeps a launcher's garden
table and allow-list (HipLauncher / GoldenLauncher wg_*) in step with the
Manager's state machine, so the gate kernels around the fused pipelines
decide every data frame of a quarantined or blocked subscriber.

The Manager stays the authority; this is the push side the reference leaves
open (SetEBPFMaps, pkg/walledgarden/manager.go:173-180 — it has no
walled_garden.c to push to)."""
from __future__ import annotations

import logging
from typing import Dict

from ..dataplane import abi
from ..dataplane.packets import ip2u32, mac_bytes
from .manager import STATE_BLOCKED, STATE_WALLED, Entry, Manager

log = logging.getLogger(__name__)

_GATE_STATE = {STATE_WALLED: abi.WG_WALLED, STATE_BLOCKED: abi.WG_BLOCKED}


def allowed_keys(manager: Manager):
    """manager.allowed_dests as the launcher's (ip, port, proto) ints."""
    return [(ip2u32(ip), port, proto)
            for ip, port, proto in list(manager.allowed_dests)]


def attach_dataplane(manager: Manager, launcher,
                     redirect_ports=abi.WG_DEFAULT_REDIRECT_PORTS):
    """Push the garden into `launcher` and keep it there: the allow-list
    now and after every allow_destination, the entries already present,
    and every later state change.  WALLED and BLOCKED entries with an
    address sit in the device table; activation, removal and TTL expiry
    take them out.  Returns the hook (already registered) for tests."""
    by_mac: Dict[str, int] = {}          # the address each MAC is gated at

    def push_config():
        launcher.wg_set_config(allowed_keys(manager), redirect_ports)

    def hook(entry: Entry):
        if not entry.ip:
            return
        ip = ip2u32(entry.ip)
        old = by_mac.get(entry.mac)
        if old is not None and old != ip:
            launcher.wg_remove([old])    # re-quarantined at a new address
            del by_mac[entry.mac]
        # remove() and expiry notify with the entry's last state: what the
        # manager tracks now decides
        state = _GATE_STATE.get(manager.state_of(entry.mac))
        try:
            if state is None:
                launcher.wg_remove([ip])
                by_mac.pop(entry.mac, None)
            else:
                launcher.wg_set([(ip, mac_bytes(entry.mac), state)])
                by_mac[entry.mac] = ip
        except RuntimeError as e:        # table full: say so, keep running
            log.warning("walled garden: %s", e)

    push_config()
    manager.on_destinations_changed(push_config)
    manager.set_dataplane_hooks(hook)
    # adopt anything already quarantined or blocked
    with manager._lock:
        present = list(manager.entries.values())
    for e in present:
        hook(e)
    return hook
