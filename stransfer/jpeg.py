"""Alias of styletransfer_amd.jpeg (drop-in module name)."""
import sys as _sys

from styletransfer_amd import jpeg as _m

_sys.modules[__name__] = _m
