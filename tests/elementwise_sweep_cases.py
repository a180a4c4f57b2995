"""Case tables of the elementwise sweeps (csrc/elementwise.hip: the layout pair either side of every model pass, column copies and adds,
convert, SiLU, the timestep sinusoid and the fused sampler step), shared by tests/test_gpu_elementwise_sweeps.py (which launches them)
and the CPU check in tests/test_host_logic.py (which redoes the arithmetic each case is named for: tile counts against the block cap of
the transposes, work items against the cap of the grid-stride loops).  Plain data and CPU references, no device needed.

The launch geometry restated from the source:
  transposes : one block per [32 channels x 64 pixels] tile, at most LAYOUT_MAX_BLOCKS blocks; further tiles are walked in a loop
  the rest   : GRID_CAP blocks of BLOCK lanes at most, one work item per lane and trip (a 16-byte vector, an element, a float4)"""
import math

import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LAYOUT_TILE_C, LAYOUT_TILE_P, LAYOUT_MAX_BLOCKS = 32, 64, 4096
BLOCK, GRID_CAP = 256, 2048
ONE_TRIP = BLOCK * GRID_CAP             # 524288 work items: one more takes a second trip of a grid-stride loop


def vec(dtype):
    return 4 if dtype == torch.float32 else 8


def trips(work):
    """trips of the grid-stride loop that the busiest lane makes over `work` items"""
    grid = max(1, min(GRID_CAP, -(-work // BLOCK)))
    return -(-work // (grid * BLOCK))


# ------------------------------------------------------------------------------------------------ layout pair
def layout(C, Cpad, shape, why):
    return dict(C=C, Cpad=Cpad, shape=shape, why=why)


LAYOUT = [
    layout(5, 8, (2, 3, 6, 10), "the shape of test_layout_roundtrip_and_concat, now exact"),
    layout(32, 40, (1, 2, 7, 9), "the second channel tile is padding only: columns 32..39 are +0"),
    layout(33, 40, (2, 1, 5, 13), "HW = 65: a one-pixel second pixel tile, a one-channel second channel tile"),
    layout(31, 32, (1, 2, 9, 7), "HW = 63"),
    layout(64, 64, (1, 1, 8, 8), "exact tiles, no edge"),
    layout(4, 8, (1, 1, 1, 1), "one pixel"),
    layout(33, 40, (1, 1, 3, 43691), "HW = 131073: 2049 x 2 tiles, above the block cap: blocks walk to a second tile"),
]
LAYOUT_WALK = LAYOUT[-1]
LAYOUT_LD_EXTRA = 16                    # ldo = Cpad + 16, ldi = C + 16 (whole vectors in every type)


def layout_id(c):
    B, F, H, W = c["shape"]
    return f"C{c['C']}-Cpad{c['Cpad']}-B{B}-F{F}-H{H}-W{W}"


def layout_tiles(c, to_rows=True):
    """(pixel tiles per (b, f), channel tiles, tiles in all) of a case: emo_ncfhw_to_rows tiles Cpad, emo_rows_to_ncfhw tiles C"""
    B, F, H, W = c["shape"]
    pt = -(-H * W // LAYOUT_TILE_P)
    ct = -(-(c["Cpad"] if to_rows else c["C"]) // LAYOUT_TILE_C)
    return pt, ct, B * F * pt * ct


def layout_refusals(c):
    """(entry, overrides of the arguments) that must be refused with nothing launched"""
    B, F, H, W = c["shape"]
    zero = [dict(B=0), dict(C=0), dict(F=0), dict(H=0), dict(W=0)]
    return ([("to_rows", dict(Cpad=c["C"] - 1, ldo=c["Cpad"])), ("to_rows", dict(ldo=c["Cpad"] - 1))] + [("to_rows", z) for z in zero] +
            [("to_ncfhw", dict(ldi=c["C"] - 1))] + [("to_ncfhw", z) for z in zero])


def rounding_specials(dtype):
    """f32 values whose cast to `dtype` is decided by the rounding: ties that go to the even neighbour both ways, the neighbours of a
    tie, the largest finite value, the tie above it (which rounds to infinity) and the last value below that tie (which does not)"""
    if dtype == torch.float32:
        return torch.tensor([0.0, -0.0, 1.0, -1.0, torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max], dtype=torch.float32)
    fi = torch.finfo(dtype)
    mant = 10 if dtype == torch.float16 else 7
    ulp1 = 2.0 ** -mant
    top = fi.max
    half_ulp_top = top * (2.0 ** -(mant + 1)) / (2 - ulp1)
    v = [1 + ulp1 / 2, 1 + 3 * ulp1 / 2, -(1 + ulp1 / 2), -(1 + 3 * ulp1 / 2), 1 + ulp1 / 2 + 2.0 ** -23, 1 + ulp1 / 2 - 2.0 ** -23,
         top + half_ulp_top, -(top + half_ulp_top), top + half_ulp_top * (1 - 2.0 ** -12), top, 0.0, -0.0]
    return torch.tensor(v, dtype=torch.float64).float()


CONCAT_M, CONCAT_WIDTHS = 37, [(16, 24), (8, 8), (320, 640)]


# ------------------------------------------------------------------------------------------------ timestep sinusoid
TS_DIMS = (2, 3, 320, 321, 1280)
TS_FLIPS = (False, True)
TS_INT = [0, 1, 261, 500, 981, 999]
TS_FRAC = [978.6, 500.5, 0.25, 13.875]          # the fractional timesteps of test_timestep_embedding_f32
TS_WALK = dict(B=1639, dim=321)                 # 526119 elements: a second trip
TS_TOL = dict(rtol=1e-5, atol=2e-5)             # tests/test_gpu_sched_kernel.py: the project's figure for this kernel in f32


def ts_walk_timesteps():
    return (torch.arange(TS_WALK["B"], dtype=torch.int64) * 7) % 1000


def ts_freqs(dim, max_period=10000):
    """the constant f32 table the models hand the kernel (embeddings.py:46-50 with freq_shift 0)"""
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half)


def ts_reference(ts, dim, flip):
    """embeddings.py:46-63 with the angle as the device forms it - ONE f32 multiply, so its bits are the device's - and sin / cos of
    that angle in f64: [sin | cos], [cos | sin] with flip, and a zero column when dim is odd.  f64 (B, dim)."""
    ang = (ts.float()[:, None] * ts_freqs(dim)[None, :]).double()
    s, c = torch.sin(ang), torch.cos(ang)
    emb = torch.cat([c, s], -1) if flip else torch.cat([s, c], -1)
    if dim % 2 == 1:
        emb = torch.cat([emb, torch.zeros(emb.shape[0], 1, dtype=torch.float64)], -1)
    return emb


# ------------------------------------------------------------------------------------------------ SiLU
SILU_SIZES = (1, 255, 257, 1048581)             # the last: a third trip with a ragged tail
SILU_SPECIALS = [0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4]     # x on the positive side, zero or a tiny negative on the other


# ------------------------------------------------------------------------------------------------ sampler step
SCHED_SMALL = [     # (C, F, HW): n % 4 == 0 every time, so aligned bases take the float4 path
    (4, 3, 1), (4, 3, 2), (4, 2, 3),            # HW < 4: several frame changes inside one vector, wrap from frame F - 1 to 0
    (4, 1, 5), (8, 1, 1),                       # F = 1: every pixel wrap returns to frame 0
]
SCHED_LARGE = [
    (4, 3, 174771),                             # n = 2097252, n / 4 = 524313: second trip of the float4 loop, HW % 4 = 3
    (3, 1, 174763),                             # n = 524289, odd: second trip of the per-element loop
]
SCHED_GUIDANCE = (7.5, 1.0)
SCHED_TOL = dict(rtol=2e-5, atol=2e-5)          # tests/test_gpu_sched_kernel.py, against f64
SCHED_COEF = dict(a=0.8, b=-0.3, c_x=0.95, s_next=0.37)
SCHED_LMS = dict(c=[0.9, -0.4, 0.2, -0.05], slot=[3, 2, 1, 0])       # LMS order 4: slot 3 written, 2 / 1 / 0 read
SCHED_NO_RING = dict(c=[0.9, 0.0, 0.0, 0.0], slot=[-1, -1, -1, -1])
SCHED_SEED, SCHED_STEP, SCHED_C_NOISE = 11, 4, 0.7
SCHED_DRAWS = dict(shape=(4, 3, 341), seeds=(11, 0x9E3779B9), steps=(0, 4, 999))    # HW % 4 = 1: the float4 path, 4092 draws per pair
SCHED_MISALIGNED = ("lat", "noise_pred", "lat_in")


def sched_id(s):
    return "C%d-F%d-HW%d" % s


# ------------------------------------------------------------------------------------------------ second trips of the other entries
COPY_ADD_WALK = dict(M=4099, C=512, ld=520)                 # f32: 4099 * 128 = 524672 vectors
ADD_PERIODIC_WALK = dict(P=7, periods=9363, C=64)           # bf16: M = 65541 rows, 65541 * 8 = 524328 vectors
CONVERT_WALK = 1048581
ACCUMULATE_WALK = dict(nf=3, C=4, HW=43700, F=3, frames=[2, -1, 0], counter=[1.0, 0.0, 1.0])     # 524400 elements
