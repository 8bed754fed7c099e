"""Float64 restatements of MRWaveGlow's plumbing in plain torch, shared by the CPU and the GPU tests (this directory is on sys.path):
the Haar split and merge, the linear upsampling (torch.nn.functional.interpolate itself, on float64), the packing of the per-level
latents, and the fp32 fma-chain bound the upsampling kernels are held to.  Nothing here launches a kernel or reads the upstream
reference; test_mrwaveglow_cpu.py pins these to the reference's own class."""
import torch
import torch.nn.functional as Fn

U32 = 2.0 ** -24      # unit roundoff of fp32


def haar_split64(x):
    """x [B, c, T] -> (diff, avg) over the channel pairs (2i, 2i + 1)"""
    x0, x1 = x[:, ::2], x[:, 1::2]
    return x1 - x0, (x0 + x1) * 0.5


def haar_merge64(avg, diff):
    """(avg, diff) [B, c/2, T] -> [B, c, T] with z0 = avg - diff / 2 at channel 2i and z1 = avg + diff / 2 at 2i + 1"""
    z0, z1 = avg - diff * 0.5, avg + diff * 0.5
    return torch.stack([z0, z1], 2).reshape(avg.size(0), -1, avg.size(2))


def upsample64(h, s, T):
    """h [B, n_mels, F] (float64) -> the first T columns of its linear interpolation by the integer factor s"""
    return Fn.interpolate(h, scale_factor=s, mode="linear")[..., :T]


def upsample_weights64(s, F, T):
    """[T, F] float64: the weights by which column t reads frame f, formed from the integers of the definition (source position
    (2t + 1 - s) / (2s), clamped at both ends) -- the |a_i b_i| of the bound below."""
    W = torch.zeros(T, F, dtype=torch.float64)
    for t in range(T):
        p = 2 * t + 1 - s
        if p < 0:
            W[t, 0] = 1.0
            continue
        i0, r = divmod(p, 2 * s)
        i1 = min(i0 + 1, F - 1)
        W[t, i0] += (2 * s - r) / (2 * s)
        W[t, i1] += r / (2 * s)
    return W


def fma_bound(n, abs_terms):
    """the project's bound of an fp32 fma chain of n terms: (n + 3) 2^-24 sum |a_i b_i|"""
    return (n + 3) * U32 * abs_terms


def split_sizes(n_group, levels):
    """channels of the per-level latents, in the order they are emitted: n_group / 2, / 4, ..., and the prior's"""
    sizes, c = [], n_group
    for _ in range(levels - 1):
        c //= 2
        sizes.append(c)
    return sizes + [c]


def pack64(parts):
    """[B, c_l, T] tensors -> [B, T * sum(c_l)]: cat(., 1).transpose(1, 2).contiguous().view(B, -1)"""
    return torch.cat(parts, 1).transpose(1, 2).contiguous().view(parts[0].size(0), -1)


def unpack64(z, n_group, sizes):
    """[B, T * n_group] -> its [B, c_l, T] parts"""
    return [p.contiguous() for p in z.view(z.size(0), -1, n_group).transpose(1, 2).split(sizes, 1)]


def analysis64(x, n_group, levels):
    """the model's forward pass without any flow: audio [B, N] -> latent [B, N]"""
    x = x.view(x.size(0), -1, n_group).transpose(1, 2)
    parts = []
    for _ in range(levels - 1):
        d, x = haar_split64(x)
        parts.append(d)
    return pack64(parts + [x])


def synthesis64(z, n_group, levels):
    """the model's reverse pass without any flow: latent [B, N] -> audio [B, N]"""
    *diffs, x = unpack64(z, n_group, split_sizes(n_group, levels))
    for d in reversed(diffs):
        x = haar_merge64(x, d)
    return x.transpose(1, 2).contiguous().view(z.size(0), -1)
