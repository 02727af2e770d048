"""Transparent substrate (smrt/substrate/transparent.py): nothing comes back from below the last layer -- the same
radiation as no substrate at all, without the "optically shallow snowpack" warning of the iterative first-order solver."""
from ..interface.transparent import Transparent as _TransparentInterface
from .rough import InterfaceSubstrate


class Transparent(InterfaceSubstrate):
    interface_class = _TransparentInterface

    def _below(self, frequency):   # (no permittivity is needed: the interface ignores its media)
        return 1.0
