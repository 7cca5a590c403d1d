"""numpy restatement of downsample_method APPROX_VOXELGRID (include/apdgicp_hip.h, AV1 .. AV7: pcl::ApproximateVoxelGrid<PointXYZI>::applyFilter,
PCL 1.10, as published; PCL is not installed here): the expected values of tests/test_approx_voxel.py and tests/test_cpp_approx_voxel.py,
and the fixtures both use.

np_approx_voxel is the literal loop: one point after the other, a table of 512 entries, every fp32 operation a numpy float32 operation and
no addition in another order than the loop's.  np_approx_voxel_sorted is the form the device runs (riv-slam_amd/csrc/apd_approx_voxel.hpp:
stable sort by hash, runs, a scan over the evicting points) written independently of the loop; tests/test_approx_voxel_cpu.py holds the two
against each other on every fixture."""
import numpy as np

F32 = np.float32
HIST = 512
INT_MIN = -2 ** 31


def voxel_indices(cloud, leaf):
    """AV1 / AV2 per point (elementwise, nothing is added up here): int64 [n, 3] holding int32 values; what an int cannot hold is INT_MIN"""
    inv = F32(1.0) / np.broadcast_to(np.asarray(leaf, dtype=F32), (3,))
    assert inv.dtype == F32
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(np.asarray(cloud[:, :3], dtype=F32) * inv[None, :])
    assert v.dtype == F32
    ok = (v >= F32(-2.0 ** 31)) & (v < F32(2.0 ** 31))
    out = np.full(v.shape, INT_MIN, dtype=np.int64)
    out[ok] = v[ok].astype(np.int64)
    return out


def voxel_hash(ijk):
    """AV3: (ix*7171 + iy*3079 + iz*4231) & 511 in 32-bit unsigned arithmetic"""
    u = np.asarray(ijk, dtype=np.int64) & 0xFFFFFFFF
    return (((u[..., 0] * 7171 + u[..., 1] * 3079 + u[..., 2] * 4231) & 0xFFFFFFFF) & (HIST - 1)).astype(np.int64)


def takes_part(cloud):
    """AV7: a point with a non-finite coordinate takes no part"""
    return np.isfinite(np.asarray(cloud[:, :3], dtype=F32)).all(1)


def np_approx_voxel(cloud, leaf):
    """The literal loop.  cloud: [n, 4] float32 {x, y, z, intensity}.  Returns (out [n_out, 4] float32, ijk [n, 3] the voxel of every point,
    emitter [n_out]: the index of the input point that caused the flush, -1 for the final flush)."""
    cloud = np.ascontiguousarray(cloud, dtype=F32)
    ijk = voxel_indices(cloud, leaf)
    hsh = voxel_hash(ijk)
    part = takes_part(cloud)
    vox = [None] * HIST
    count = [0] * HIST
    cent = np.zeros((HIST, 4), dtype=F32)
    out, emitter = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for cp in range(len(cloud)):
            if not part[cp]:
                continue
            h = int(hsh[cp])
            v = (int(ijk[cp, 0]), int(ijk[cp, 1]), int(ijk[cp, 2]))
            if count[h] > 0 and vox[h] != v:                      # AV4: flush
                out.append(cent[h] / F32(count[h]))
                emitter.append(cp)
                count[h] = 0
                cent[h] = F32(0)
            vox[h] = v
            count[h] += 1
            cent[h] = cent[h] + cloud[cp]                          # four fp32 additions, component by component
        for h in range(HIST):                                      # AV5
            if count[h] > 0:
                out.append(cent[h] / F32(count[h]))
                emitter.append(-1)
    res = np.array(out, dtype=F32).reshape(-1, 4)
    return res, ijk, np.array(emitter, dtype=np.int64)


def np_approx_voxel_sorted(cloud, leaf):
    """The sort-and-scan form, independent of the loop above: returns out [n_out, 4] float32"""
    cloud = np.ascontiguousarray(cloud, dtype=F32)
    n = len(cloud)
    ijk = voxel_indices(cloud, leaf)
    key = np.where(takes_part(cloud), voxel_hash(ijk), HIST)
    order = np.argsort(key, kind="stable")
    order = order[key[order] < HIST]
    m = len(order)
    if m == 0:
        return np.zeros((0, 4), dtype=F32)
    k, v = key[order], ijk[order]
    first = np.ones(m, dtype=bool)
    first[1:] = k[1:] != k[:-1]
    head = first.copy()
    head[1:] |= (v[1:] != v[:-1]).any(1)
    evict = np.zeros(n, dtype=np.int64)
    evict[order[head & ~first]] = 1
    before = np.cumsum(evict) - evict                              # evicting points in front of every input point
    n_evict = int(evict.sum())
    occ = np.zeros(HIST, dtype=np.int64)
    occ[k[first]] = 1
    occ_below = np.cumsum(occ) - occ
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], m)
    out = np.zeros((len(starts), 4), dtype=F32)
    seen = np.zeros(len(starts), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, e in zip(starts, ends):
            acc = np.zeros(4, dtype=F32)
            for j in order[s:e]:
                acc = acc + cloud[j]
            slot = before[order[e]] if e < m and k[e] == k[s] else n_evict + occ_below[k[s]]
            assert not seen[slot]
            seen[slot] = True
            out[slot] = acc / F32(e - s)
    assert seen.all() and len(starts) == n_evict + int(occ.sum())
    return out


def checksum(a):
    """what tests/cpp/test_approx_voxel.cpp prints: FNV-1a (64 bit) over the bytes"""
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------ fixtures (name -> (cloud [n, 4] float32, leaf)), each a pure function
# Block sizes of the device path: 256 (AV_BLK), 1024 (SCAN_BLK), 4096 (SCAN_BLK * SCAN_ITEMS = MAP_RS_TILE)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193)
BIG_N = 2 ** 17 + 1


def _with_intensity(xyz, rng):
    return np.ascontiguousarray(np.concatenate([xyz.astype(F32), rng.uniform(0, 40, (len(xyz), 1)).astype(F32)], 1))


def sized_cloud(n, seed=11):
    """n points uniform in [-3, 3]^3: at leaf 0.5 about 1700 voxels share the 512 entries"""
    rng = np.random.default_rng(seed + n)
    return _with_intensity(rng.uniform(-3, 3, (max(n, 1), 3)), rng)[:n]   # (n = 0: an empty slice that keeps the 16-byte row stride)


def collisions_cloud():
    rng = np.random.default_rng(3)
    return _with_intensity(rng.uniform(-2, 2, (3000, 3)), rng)


def alternation_cloud():
    """voxels (0, 0, 0) and (512, 0, 0) share entry 0 at leaf 1: visited A, B, A, B, ..."""
    rng = np.random.default_rng(4)
    xyz = rng.uniform(0.05, 0.95, (600, 3))
    xyz[1::2, 0] += 512.0
    return _with_intensity(xyz, rng)


LONG_RUN = 2100  # > 2 * SCAN_BLK: one lane adds across every block edge


def long_runs_cloud(shuffled=False):
    """four voxels of leaf 1 in four different entries, the points of each contiguous; the first run is LONG_RUN points long"""
    rng = np.random.default_rng(5)
    parts = []
    for corner, m in (((0, 0, 0), LONG_RUN), ((1, 0, 0), 700), ((0, 1, 0), 300), ((-1, -1, 2), 17)):
        parts.append(np.asarray(corner, dtype=np.float64)[None, :] + rng.uniform(0.05, 0.95, (m, 3)))
    c = _with_intensity(np.concatenate(parts), rng)
    if shuffled:
        c = np.ascontiguousarray(c[np.random.default_rng(6).permutation(len(c))])
    return c


def sparse_cloud():
    """every point in a voxel of its own (a jittered lattice of pitch 3 at leaf 0.5)"""
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(np.arange(-6, 6), np.arange(-5, 5), np.arange(-4, 4), indexing="ij"), -1).reshape(-1, 3) * 3.0
    g = g[rng.permutation(len(g))] + rng.uniform(0.05, 0.45, (len(g), 3))
    return _with_intensity(g, rng)


def faces_cloud():
    """points exactly on voxel faces (multiples of the leaf 0.25, negative ones included), several per voxel"""
    rng = np.random.default_rng(8)
    xyz = rng.integers(-9, 9, (1500, 3)).astype(np.float64) * 0.25
    xyz[::3] += rng.uniform(0, 0.25, (500, 3))
    return _with_intensity(xyz, rng)


def negative_cloud():
    rng = np.random.default_rng(9)
    return _with_intensity(rng.uniform(-40, -0.01, (2000, 3)), rng)


def overflow_cloud():
    """x * inv = 3e9 and beyond on the positive side, -3e9 on the other, and an infinite product of finite factors: all INT_MIN"""
    rng = np.random.default_rng(10)
    c = _with_intensity(rng.uniform(-2, 2, (400, 3)), rng)
    c[5, 0], c[77, 1], c[200, 2], c[201, 0], c[333, 0] = 3.0e8, 3.0e8, -3.0e8, 3.0e38, 2.5e8
    return c


def holes_cloud():
    rng = np.random.default_rng(12)
    c = _with_intensity(rng.uniform(-2, 2, (2500, 3)), rng)
    bad = rng.choice(len(c), 60, replace=False)
    c[bad[:20], 0], c[bad[20:40], 1], c[bad[40:50], 2], c[bad[50:], 0] = np.nan, np.inf, -np.inf, np.nan
    c[0, 0] = c[-1, 2] = np.nan
    return c, np.sort(np.append(bad, [0, len(c) - 1]))


_FIXTURES = {}


def fixtures():
    if _FIXTURES:
        return _FIXTURES
    f = _FIXTURES
    f.update({f"n{n}": (sized_cloud(n), 0.5) for n in SIZES})
    f["collisions"] = (collisions_cloud(), 0.5)
    f["alternation"] = (alternation_cloud(), 1.0)
    f["long_runs"] = (long_runs_cloud(), 1.0)
    f["long_runs_shuffled"] = (long_runs_cloud(True), 1.0)
    f["sparse"] = (sparse_cloud(), 0.5)
    f["faces"] = (faces_cloud(), 0.25)
    f["negative"] = (negative_cloud(), 0.7)
    f["anisotropic"] = (sized_cloud(3001, 21), (0.3, 0.9, 1.7))
    f["overflow"] = (overflow_cloud(), 0.1)
    f["holes"] = (holes_cloud()[0], 0.5)
    return f


def big_cloud():
    """BIG_N points: more than one block of every kernel and 33 scan tiles"""
    return sized_cloud(BIG_N, 31), 0.5


_EXPECTED = {}


def expected(name):
    """the literal loop's result on a fixture, computed once per process and handed out read-only"""
    if name not in _EXPECTED:
        cloud, leaf = big_cloud() if name == "big" else fixtures()[name]
        out, ijk, em = np_approx_voxel(cloud, leaf)
        for a in (cloud, out, ijk, em):
            a.setflags(write=False)
        _EXPECTED[name] = (cloud, leaf, out, ijk, em)
    return _EXPECTED[name]
