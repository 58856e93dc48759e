"""What the parameter-EMA tests share: the error bound of one fp32 update against the formula in fp64, and a
reference average evaluated in fp64.

One update ``ema + w * (p - ema)`` makes three fp32 roundings (difference, product, sum) besides the rounding of
``w = 1 - decay`` to fp32.  With ``M = max(|ema_old|, |p_new|)`` per element every intermediate is at most 2M, so the
absolute error against the exact formula is at most 9 * 2^-24 * M < 2^-20 * M.  The recursion contracts errors by
``decay`` per step, so after n updates the error is at most min(n, 1 / (1 - decay)) * 2^-20 * M, with M the largest
magnitude the parameter took over the run (an average never exceeds it)."""
import torch

EPS = 2.0 ** -20


def one_step_bound(ema_old: torch.Tensor, p_new: torch.Tensor) -> torch.Tensor:
    return EPS * torch.maximum(ema_old.double().abs(), p_new.double().abs())


def n_step_bound(n: int, decay: float, mag: torch.Tensor) -> torch.Tensor:
    return min(float(n), 1.0 / (1.0 - decay)) * EPS * mag.double()


def ema_fp64(ema_old: torch.Tensor, p_new: torch.Tensor, decay: float) -> torch.Tensor:
    e, p = ema_old.double(), p_new.double()
    return e + (1.0 - decay) * (p - e)


class Ema64:
    """The definition's average of a list of fp32 tensors, in fp64: started as a copy before the first step,
    ``update`` after every step; tracks the largest magnitude seen for the bound."""

    def __init__(self, tensors, decay):
        self.decay = decay
        self.avg = [t.detach().double().clone() for t in tensors]
        self.mag = [a.abs() for a in self.avg]
        self.n = 0

    def update(self, tensors):
        for i, t in enumerate(tensors):
            t = t.detach().double()
            self.avg[i] = self.avg[i] + (1.0 - self.decay) * (t - self.avg[i])
            self.mag[i] = torch.maximum(self.mag[i], t.abs())
        self.n += 1

    def check(self, emas, what=""):
        for i, e in enumerate(emas):
            err = (e.detach().double().cpu() - self.avg[i].cpu()).abs()
            bound = n_step_bound(self.n, self.decay, self.mag[i].cpu())
            worst = float((err - bound).max())
            assert worst <= 0.0, (what, i, float(err.max()), float(bound.max()))
