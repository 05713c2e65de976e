"""numpy restatement of the device-noise contract, written from the contract text and the Philox
paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), not from the kernel.

For image seed s, step index i, tag and element e of the image:
  block q = e >> 2:  (r0, r1, r2, r3) = philox4x32_10(counter = (q, i, tag, 0), key = (s & 0xffffffff, s >> 32))
  (r0, r1) -> elements 4q, 4q+1 (cos, sin) and (r2, r3) -> 4q+2, 4q+3, with
  u1 = ((r >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r >> 8) * 2^-24 in [0, 1),  z = sqrt(-2 ln u1) * {cos, sin}(2 pi u2).
u1 and u2 are exact in fp32, so the float64 evaluation below starts from exactly the kernel's inputs.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr: np.ndarray, key) -> np.ndarray:
    """ctr: uint32 [N, 4]; key: two 32-bit words; returns uint32 [N, 4]."""
    c = [np.asarray(ctr)[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]         # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def noise_bits(seed: int, step: int, tag: int, n_per_image: int) -> np.ndarray:
    """uint32 [4 * ceil(n_per_image / 4)]: the words of every block of one image."""
    nq = (int(n_per_image) + 3) // 4
    ctr = np.zeros((nq, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nq, dtype=np.uint32)
    ctr[:, 1] = np.uint32(step)
    ctr[:, 2] = np.uint32(tag)
    seed = int(seed)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)


def normals_from_bits(bits: np.ndarray):
    """(z float64 [len(bits)], radius float64 [len(bits)]): radius = sqrt(-2 ln u1) of the element's pair."""
    r = np.asarray(bits, dtype=np.uint32).reshape(-1, 2)
    u1 = ((r[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (r[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)
    return z, np.repeat(rad, 2)


def noise_normals(seed: int, step: int, tag: int, n_per_image: int):
    """(z, radius) float64 [n_per_image] of one image."""
    z, rad = normals_from_bits(noise_bits(seed, step, tag, n_per_image))
    return z[:n_per_image], rad[:n_per_image]


# Random123's published known-answer vectors for philox4x32-10: (counter, key, result)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def ks_pvalue_normal(z: np.ndarray) -> tuple:
    """(D, p): two-sided Kolmogorov-Smirnov statistic of z against N(0,1) and its asymptotic p-value
    Q(lambda) = 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lambda^2), lambda = (sqrt(N) + 0.12 + 0.11 / sqrt(N)) D (Stephens' small-sample
    correction, which is nothing at the N of these tests, over a million)."""
    import math
    x = np.sort(np.asarray(z, dtype=np.float64))
    n = x.size
    cdf = 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    p = 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))
    return d, min(1.0, max(0.0, p))


def _erf(x: np.ndarray) -> np.ndarray:
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()
