"""Independent reference for the fp8 cast kernels: round-to-nearest-even onto the finite values of OCP
e4m3fn (fmt 0) / e5m2 (fmt 1), built from the 256-entry decode table alone (no fp8 arithmetic), plus a
monotone ordering of the sign-magnitude codes for "code distance" assertions.  Runs on CPU and GPU."""
import torch

FMT_DTYPE = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
FMT_MAX = {0: 448.0, 1: 57344.0}

_tables = {}


def decode_table(fmt: int, device="cpu") -> torch.Tensor:
    """float64 value of each of the 256 codes (NaN / inf codes included)."""
    return torch.arange(256, dtype=torch.uint8).view(FMT_DTYPE[fmt]).double().to(device)


def _mids(fmt: int, device):
    key = (fmt, str(device))
    if key not in _tables:
        pos = decode_table(fmt, device)[:128]
        pos = pos[torch.isfinite(pos)]                  # codes 0 .. n-1: +0 .. +fmax, strictly increasing
        assert float(pos[-1]) == FMT_MAX[fmt] and bool((pos[1:] > pos[:-1]).all())
        _tables[key] = (pos[:-1] + pos[1:]) / 2         # exact in float64 (neighbours differ by one fp8 ulp)
    return _tables[key]


def ref_quant(v: torch.Tensor, fmt: int) -> torch.Tensor:
    """uint8 code of the finite fp8 value nearest to each (already scaled) float64 ``v``: ties to the even
    code, |v| saturates at fmax (inf included), the sign bit is kept for -0.  NaN inputs are not defined here
    (callers mask them out)."""
    assert v.dtype == torch.float64
    mids = _mids(fmt, v.device)
    a = v.abs().clamp(max=FMT_MAX[fmt])
    c = torch.searchsorted(mids, a.reshape(-1).contiguous()).reshape(a.shape)    # midpoints strictly below |v|
    tie = mids[c.clamp(max=mids.numel() - 1)] == a                              # |v| exactly half way: c or c + 1
    c = c + (tie & (c % 2 == 1)).to(c.dtype)
    sign = torch.signbit(v).to(c.dtype) << 7
    return (c | sign).to(torch.uint8)


def code_order(c: torch.Tensor) -> torch.Tensor:
    """Sign-magnitude fp8 codes -> integers that increase with the decoded value (+0 and -0 both 0), so
    |code_order(a) - code_order(b)| counts the representable steps between two codes."""
    c = c.view(torch.uint8).to(torch.int32)
    mag = c & 0x7F
    return torch.where((c & 0x80) != 0, -mag, mag)


def all_bf16_patterns(device="cpu") -> torch.Tensor:
    """Every bf16 bit pattern once, in bit order, as a [65536] bf16 tensor."""
    return torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(torch.bfloat16)
