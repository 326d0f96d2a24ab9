"""The dynamic LDS a launch of the DTW wavefront kernels asks for, restated from soundsym_amd/csrc/dtw_wave.hpp -- TEST
INFRASTRUCTURE.  The spot kernels and the spotter's forward kernel take fbCap * 12 + ringRows * wave_ld(dimr) * 8 bytes:
a hand-off row of (f64, u32) per target frame and the ring of target frames.  Above 64 KiB a launch needs
hipFuncSetAttribute(MaxDynamicSharedMemorySize) first, so the tests name the side of 65536 every case is on."""

LIMIT = 64 * 1024          # what a kernel may ask for without the attribute


def wave_dimr(dim):
    return 14 if dim <= 14 else 16 if dim <= 16 else 40 if dim <= 40 else 64


def wave_ld(dimr):
    return dimr if dimr % 4 == 2 else dimr + 2


def wave_fb_cap(max_fb):
    return (max(max_fb, 1) + 1) & ~1          # even: an odd longest target takes one entry more


def wave_ring_rows(max_fb):
    return 64 if max_fb <= 64 else 128


def spot_lds_bytes(dim, max_fb):
    """Bytes of one launch whose longest target has max_fb frames of dim values."""
    return wave_fb_cap(max_fb) * 12 + wave_ring_rows(max_fb) * wave_ld(wave_dimr(dim)) * 8


# (dim, frames of the longest target, above 64 KiB): both sides of every crossing, at both ends of each DIMR's range of
# dims, the largest launch there is and the largest that stays below.  fbCap is even, so the crossings sit at odd lengths:
# 1877 and 3925 frames already take what 1878 and 3926 take.
CROSSINGS = (
    [(d, fb, fb > 64) for d in (64, 41) for fb in (64, 65, 130)] +                     # 34560 | 68376, 69144
    [(d, fb, fb > 1876) for d in (40, 17) for fb in (1876, 1877, 1878)] +              # 65520 | 65544, 65544
    [(d, fb, fb > 3924) for d in (16, 15) for fb in (3924, 3925, 3926)] +              # 65520 | 65544, 65544
    [(64, 4096, True), (14, 4096, False)])                                             # 116736, 63488
