"""Per-subscriber traffic accounting: the glue between the dataplane's
device-side counters and the RADIUS accounting records."""
from .traffic import TrafficAccounting

__all__ = ["TrafficAccounting"]
