"""What the FusedLAMB tests share: the definition evaluated in fp64 over a list of logical tensors, the same code in
fp32 torch ops ("the fp32 composite"), and the tolerance derived from the two.

Tolerance.  ``e_ref`` = max abs error of the fp32 composite against the fp64 reference on the same inputs.  A tested
path passes when its max abs error against the fp64 reference is at most ``max(4 * e_ref, 2^-22 * max|x|)`` -- the
factor 4 allows for a different summation order in the norms, the floor is 2 ulp of the largest value -- applied to
the parameters and to each moment with its own ``e_ref`` and its own largest magnitude.

The sums of squares (``trust_sums``) get the floor that fp32 summation itself implies: a sum of n non-negative terms
whose every term passes through at most d additions is within d * 2^-24 of exact, relative, in any order.  The kernels
add at most 128 terms per thread serially, then 6 + 2 tree levels per block and at most ceil(count / 256) + 8 for the
row; the squares and u itself add a few more roundings per term.  d <= 256 covers every shape the tests use, so
``|sum - ref| <= max(4 * e_ref, 2^-16 * ref)``."""
import torch

SUM_REL = 2.0 ** -16


def lamb_steps(params, grad_lists, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False,
               grad_scale=1.0, dtype=torch.float64, state=None):
    """Run ``len(grad_lists)`` LAMB steps in ``dtype`` on copies of ``params`` (a list of logical tensors).
    -> (params, exp_avgs, exp_avg_sqs, sums) with ``sums`` the last step's [n, 2] (||p||^2, ||u||^2), ``p`` before
    that step's update.  ``state``: (exp_avgs, exp_avg_sqs, steps done) to continue from."""
    b1, b2 = betas
    dev = params[0].device
    ps = [p.detach().to(dtype).clone() for p in params]
    if state is None:
        ms, vs, t0 = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], 0
    else:
        ms, vs, t0 = [m.detach().to(dtype).clone() for m in state[0]], \
            [v.detach().to(dtype).clone() for v in state[1]], state[2]
    sums = torch.zeros(len(ps), 2, dtype=dtype, device=dev)
    adapt = weight_decay != 0 or always_adapt
    for k, grads in enumerate(grad_lists):
        t = t0 + k + 1
        bc1, bc2_sqrt = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
        for i, p in enumerate(ps):
            g = grads[i].detach().to(dtype).reshape(p.shape) * grad_scale
            m, v = ms[i], vs[i]
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (m / bc1) / (v.sqrt() / bc2_sqrt + eps) + weight_decay * p
            pn, un = (p * p).sum(), (u * u).sum()
            sums[i, 0], sums[i, 1] = pn, un
            r = pn.sqrt() / un.sqrt() if (adapt and float(pn) > 0 and float(un) > 0) else 1.0
            p.sub_(u * (lr * r))
    return ps, ms, vs, sums


def reference_and_composite(params, grad_lists, **kw):
    """-> (fp64 reference, fp32 composite), each ``lamb_steps``' tuple, computed once for the tests that share them."""
    return lamb_steps(params, grad_lists, dtype=torch.float64, **kw), \
        lamb_steps(params, grad_lists, dtype=torch.float32, **kw)


def _err(xs, refs):
    return max(float((x.detach().double().cpu().reshape(-1) - r.double().cpu().reshape(-1)).abs().max())
               for x, r in zip(xs, refs))


def check(got, ref, comp, what=""):
    """``got`` = (params, exp_avgs, exp_avg_sqs, sums or None) of the tested path against the fp64 reference ``ref``
    with the composite ``comp`` setting the tolerance.  Prints every error before it asserts."""
    failed = []
    for name, g, r, c in zip(("param", "exp_avg", "exp_avg_sq"), got[:3], ref[:3], comp[:3]):
        e_ref, e = _err(c, r), _err(g, r)
        floor = 2.0 ** -22 * max(float(x.abs().max()) for x in r)
        print(f"[lamb {what}] {name}: err {e:.3e}  e_ref {e_ref:.3e}  bound {max(4 * e_ref, floor):.3e}")
        if not e <= max(4 * e_ref, floor):
            failed.append((name, e, e_ref, floor))
    if got[3] is not None:
        s, rs, cs = got[3].detach().double().cpu(), ref[3].double().cpu(), comp[3].double().cpu()
        e_ref = float((cs - rs).abs().max())
        bound = torch.clamp(SUM_REL * rs, min=4 * e_ref)
        worst = float(((s - rs).abs() / rs.clamp_min(1e-300)).max()) if float(rs.max()) > 0 else 0.0
        print(f"[lamb {what}] trust_sums: max rel err {worst:.3e}  e_ref {e_ref:.3e}  rel bound {SUM_REL:.3e}")
        if not bool(((s - rs).abs() <= bound).all()):
            failed.append(("trust_sums", worst, e_ref, SUM_REL))
    assert not failed, (what, failed)
