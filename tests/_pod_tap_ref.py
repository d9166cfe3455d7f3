"""Seeded inputs and the exact definitions for the pre-ReLU POD tap
(ops.add_relu_tap, csrc/norm.hip add_relu_tap_*), shared by test_pod_tap.py
and test_pod_tap_gpu.py.

Definitions, bf16 in and out, every value exact (no tolerance anywhere):
``z = bf16_rne(float(a) + float(b))``, ``y = z > 0 ? z : 0``,
``g = bf16_rne(float(dz) + (z > 0 ? float(dy) : 0))``; without ``dz``
``g = z > 0 ? dy : 0``, without ``dy`` ``g = dz``.
"""

import torch

import _pod_ref as R

BF = torch.bfloat16

# flat totals: tail only; one vector; one block of 2048 minus one, exactly
# one block, one block plus a 3-element tail; then two 4-D maps (the second
# sixteen blocks)
TAP_SHAPES = [(5,), (8,), (2047,), (2048,), (2051,), (3, 5, 7, 8),
              (2, 32, 32, 16)]
TAP_IDS = ["x".join(map(str, s)) for s in TAP_SHAPES]


def signed_maps(name, seed=0):
    """-> (a, b) bf16 CPU maps of _pod_ref.SHAPES[name]: ``randn + 0.1 sign``,
    both signs, no zero entry."""
    shape = R.SHAPES[name]
    g = torch.Generator().manual_seed(104729 * (R.SHAPE_IDS.index(name) + 1)
                                      + seed)
    out = []
    for _ in range(2):
        x = torch.randn(shape, generator=g)
        x = (x + 0.1 * torch.where(x >= 0, 1.0, -1.0)).to(BF)
        assert (x != 0).all()
        out.append(x)
    assert all((x < 0).any() for x in out) or name == "degenerate"
    return out[0], out[1]


# (a, b): sum exactly 0; both zero; negative and tiny; RNE ties: 1 + 2^-8
# lies halfway between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 2^-8 goes
# up to 1 + 2^-6; the same tie below zero
_PLANTS = [(1.5, -1.5), (0.0, 0.0), (2.0 ** -100, -(2.0 ** -99)),
           (1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8),
           (-1.0, -(2.0 ** -8))]
_PLANT_Z = [0.0, 0.0, -(2.0 ** -100), 1.0, 1.0 + 2.0 ** -6, -1.0]


def tap_inputs(shape, seed=0):
    """-> (a, b, dy, dz) bf16 CPU: signed randn with the planted elements at
    the front, in the middle and at the very end (inside the scalar tail where
    the total has one)."""
    total = 1
    for s in shape:
        total *= s
    g = torch.Generator().manual_seed(7 + 31 * total + seed)
    a, b, dy, dz = (torch.randn(total, generator=g).to(BF) for _ in range(4))
    where = [0, 1, total // 2, total - 1, total - 2, total // 2 + 1]
    if total < 8:  # the first four plants only
        where = [0, 1, 2, total - 1]
    assert len(set(where)) == len(where) and max(where) < total
    for i, pos in enumerate(where):
        a[pos], b[pos] = _PLANTS[i]
        assert float(a[pos]) == _PLANTS[i][0] and \
            float(b[pos]) == _PLANTS[i][1]  # the plants are bf16 values
    y, z = tap_fwd_ref(a, b)
    for i, pos in enumerate(where):
        assert float(z[pos]) == _PLANT_Z[i], (i, float(z[pos]))
    return tuple(t.reshape(shape) for t in (a, b, dy, dz))


def tap_fwd_ref(a, b):
    z = (a.float() + b.float()).to(BF)
    return torch.where(z > 0, z, torch.zeros_like(z)), z


def tap_bwd_ref(dy, dz, z):
    if dy is None:
        return dz.clone()
    if dz is None:
        return torch.where(z > 0, dy, torch.zeros_like(dy))
    m = torch.where(z > 0, dy.float(), torch.zeros_like(dy, dtype=torch.float))
    return (dz.float() + m).to(BF)
