"""Alias of styletransfer_amd.adain (drop-in module name)."""
import sys as _sys

from styletransfer_amd import adain as _m

_sys.modules[__name__] = _m
