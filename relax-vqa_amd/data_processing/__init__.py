"""Counterparts of the reference's src/data_processing modules that touch pixels or decide which rows a protocol sees
(same function names and argument meaning), running on the HIP engine."""
from . import check_greyscale  # noqa: F401
