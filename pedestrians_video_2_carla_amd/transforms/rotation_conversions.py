"""Rotation conversions the reference takes from pytorch3d 0.6.0 (absent third-party dependency; published
definitions restated). Composed of differentiable torch ops: used only OUTSIDE the fused path
(API compatibility for ``rotation_output_format='matrix'``, teacher forcing targets); the training hot path feeds the
raw 6-D tensor to the HIP pose head, which orthonormalises in-kernel.
"""
import torch
from torch import Tensor


def rotation_6d_to_matrix(d6: Tensor) -> Tensor:
    """Zhou et al. 2019: Gram-Schmidt of the two 3-vectors, third row = cross product; rows (b1, b2, b3)."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def matrix_to_rotation_6d(matrix: Tensor) -> Tensor:
    return matrix[..., :2, :].clone().reshape(matrix.shape[:-2] + (6,))


def euler_angles_to_matrix(euler_angles: Tensor, convention: str = 'XYZ') -> Tensor:
    def axis(k, a):
        c, s, o, z = torch.cos(a), torch.sin(a), torch.ones_like(a), torch.zeros_like(a)
        rows = {'X': (o, z, z, z, c, -s, z, s, c), 'Y': (c, z, s, z, o, z, -s, z, c), 'Z': (c, -s, z, s, c, z, z, z, o)}[k]
        return torch.stack(rows, -1).reshape(a.shape + (3, 3))
    m = [axis(k, euler_angles[..., i]) for i, k in enumerate(convention)]

    def mm3(a, b):       # 3x3 products as element-wise work: the synthetic data module composes (B, T, 26) of them per batch,
        return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2)      # which as a batched library GEMM took ~1 ms per call
    return mm3(mm3(m[0], m[1]), m[2])


def matrix_to_euler_angles(matrix: Tensor, convention: str = 'XYZ') -> Tensor:
    """Inverse of ``euler_angles_to_matrix(., 'XYZ')`` above, R = Rx(a0) Ry(a1) Rz(a2) (the only convention the reference
    ever asks for; any other raises): a1 = asin(R[0,2]), a0 = atan2(-R[1,2], R[2,2]), a2 = atan2(-R[0,1], R[0,0]); (..., 3, 3)
    -> (..., 3). The middle angle comes back in [-90, 90] degrees: a matrix built from a middle angle beyond that range
    returns its other Euler representation, which gives the same matrix.
    One deliberate difference from pytorch3d: R[0,2] is clamped to [-1, 1] before the asin. An orthonormalised fp32 network
    output can land one ulp outside that range, where pytorch3d returns NaN; here it is +-90 degrees. (torch.clamp lets a NaN
    through, so a missing joint still gives NaN.)"""
    if convention != 'XYZ':
        raise ValueError(f"matrix_to_euler_angles: convention '{convention}' ('XYZ' is the only one implemented)")
    if matrix.ndim < 2 or tuple(matrix.shape[-2:]) != (3, 3):
        raise ValueError(f'matrix_to_euler_angles: (..., 3, 3) expected, got {tuple(matrix.shape)}')
    a1 = torch.asin(torch.clamp(matrix[..., 0, 2], -1.0, 1.0))
    a0 = torch.atan2(-matrix[..., 1, 2], matrix[..., 2, 2])
    a2 = torch.atan2(-matrix[..., 0, 1], matrix[..., 0, 0])
    return torch.stack((a0, a1, a2), -1)
