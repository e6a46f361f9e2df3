"""The P-point position encodings restated on the CPU ("the rule"), in the reference's operation order: how a
patch's coordinates are aggregated (sample9 / sample5 / sample1 / minmax), the voxeliser, and PositionEmbeddingSine3D with n_points.
torch supplies the dtype arithmetic (f16 / bf16 ops round as the reference's do because they are the same ops); the index rules
are written out.  tests/test_pe_points_check_cpu.py holds it against tests/golden/pe_points.npz, which the reference's own functions
wrote; the GPU tests then use it where a golden would be too large to store."""
import numpy as np
import torch

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODES = {"sample9": 9, "sample5": 5, "sample1": 1, "minmax": 2}
MIN_XYZ, MAX_XYZ, VOXEL = (-15, -15, -5), (15, 15, 5), 0.1
SEED = 20251
# (E, P) pairs of the PE goldens; tokens per pair
PE_CASES = ((256, 9), (256, 5), (256, 2), (3584, 9), (3584, 5), (3584, 2))
PE_TOKENS = {256: 16, 3584: 4}


def seeded_coords(kind="f32"):
    """The [2,384,384,3] input of the coordinate goldens: about a sixth of the values outside min/max_xyz_range, a NaN on a sampled pixel
    (patch v=1, py=3, px=5: every mode sees it) and one on an unsampled pixel (v=0, py=7, px=2, y only: only minmax sees it)."""
    g = np.random.default_rng(SEED)
    x = (g.random((2, 384, 384, 3), dtype=np.float32) - 0.5) * np.array([36, 36, 12], np.float32)
    x[1, 27 * 3 + 13, 27 * 5 + 13, :] = np.nan
    x[0, 27 * 7 + 1, 27 * 2 + 2, 1] = np.nan
    return torch.from_numpy(x).to(DT[kind])


def pe_inputs(E, P, kind, continuous):
    """xyz [N,P,3] of the PE goldens: integer ids in [0, 300] (0 and 300 included), or continuous coordinates in +-15 / +-15 / +-5."""
    N = PE_TOKENS[E]
    g = np.random.default_rng(SEED + 7 * E + P + (1000 if continuous else 0))
    if continuous:
        x = (g.random((N, P, 3), dtype=np.float32) - 0.5) * np.array([30, 30, 10], np.float32)
    else:
        x = g.integers(0, 301, (N, P, 3)).astype(np.float32)
        x[0, 0, 0], x[0, 0, 1] = 0.0, 300.0
    return torch.from_numpy(x).to(DT[kind])


def sample_points(coords, n_points):
    """rows 27*py + {4,13,22} x columns 27*px + {4,13,22}, point 3*ri + ci; 5 -> points 0,2,4,6,8; 1 -> point 4, [V,14,14,3]."""
    V = coords.shape[0]
    at = (27 * torch.arange(14)[:, None] + torch.tensor([4, 13, 22])[None, :])          # [14 cells, 3 offsets]
    rows = at[:, None, :, None].expand(14, 14, 3, 3)
    cols = at[None, :, None, :].expand(14, 14, 3, 3)
    nine = coords[:, rows, cols, :].reshape(V, 14, 14, 9, 3)
    if n_points == 9:
        return nine
    if n_points == 5:
        return nine[:, :, :, 0::2, :]
    if n_points == 1:
        return nine[:, :, :, 4, :]
    raise ValueError(n_points)


def minmax_points(coords):
    """point 0 the per-axis minimum over each 27x27 patch, point 1 the maximum; NaN in the patch -> NaN."""
    V = coords.shape[0]
    p = coords[:, :378, :378, :].reshape(V, 14, 27, 14, 27, 3).float()                   # min / max of 16-bit values are exact in f32
    return torch.stack([p.amin(dim=(2, 4)), p.amax(dim=(2, 4))], dim=3).to(coords.dtype)


def aggregate(coords, mode):
    return minmax_points(coords) if mode == "minmax" else sample_points(coords, MODES[mode])


def discrete(x, lo=MIN_XYZ, hi=MAX_XYZ, voxel=VOXEL):
    """clamp (NaN kept); (x - lo) in x's dtype; / voxel in x's dtype; round half to even."""
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    x = torch.minimum(torch.maximum(x, lo_t), hi_t)
    return ((x - lo_t) / voxel).round()


def dim_t(nf, temperature=10000):
    d = torch.arange(nf, dtype=torch.float32)
    return temperature ** (2 * (d // 2) / nf)


def pe(xyz, E, n_points):
    """xyz [N,P,3] (or [N,3] with P = 1) -> [N,E] in xyz's dtype: channel c < 3*P*nf has q = c // nf, j = c % nf and holds
    sin (j even) / cos (j odd) of f32(xyz[q]) / dim_t[j]; the rest is 0."""
    N = xyz.shape[0]
    nf = E // (3 * n_points)
    arg = xyz.reshape(N, 3 * n_points, 1).float() / dim_t(nf)                            # [N, 3P, nf], f32 division
    j = torch.arange(nf)
    val = torch.where(j % 2 == 0, arg.sin(), arg.cos())
    out = torch.zeros((N, E), dtype=xyz.dtype)
    out[:, : 3 * n_points * nf] = val.reshape(N, -1).to(xyz.dtype)
    return out


def pe_f64(xyz, E, n_points):
    """The same rule with the trig correctly rounded to f32 (evaluated in f64 on the f32 quotient): what the kernels compute."""
    N = xyz.shape[0]
    nf = E // (3 * n_points)
    arg = (xyz.reshape(N, 3 * n_points, 1).float() / dim_t(nf)).double()
    j = torch.arange(nf)
    val = torch.where(j % 2 == 0, arg.sin(), arg.cos()).float()
    out = torch.zeros((N, E), dtype=xyz.dtype)
    out[:, : 3 * n_points * nf] = val.reshape(N, -1).to(xyz.dtype)
    return out


def bits(t):
    """16-bit tensor -> raw uint16 bits; f32 -> numpy f32."""
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def from_bits(a, kind):
    if kind == "f32":
        return torch.from_numpy(np.ascontiguousarray(a))
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(DT[kind])
