"""MI355X-native demix hot path of xumx-sliCQ-V2 (sliCQT -> CDAE -> phasemix |
Wiener-EM -> isliCQT) behind the reference's Separator / Unmix / NSGT_SL /
INSGT_SL module API.  The arithmetic lives in ``csrc/`` (hand-written HIP for
gfx950 behind a C ABI, ``include/xumx_slicq_hip.h``); this package holds the
host-side plan builder and the ``nn.Module`` mirrors of the reference surface
(``separator``, ``inference``, ``cadenza.separate_sources`` for overlapped, cross-faded segments).
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the public names of ``separator`` without importing the HIP library (and torch) when the package is imported
    if name in ("Separator", "StreamSession", "StreamGrid", "streamed_loop", "stream_steps"):
        from . import separator
        return getattr(separator, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
