"""The host side of one sampler step, once: the plan of a schedule's model calls (`step_plan`) and the STEP record of one of them
(`step_record`), for the serving batcher and the pipeline's fused loop alike - a served request carries the bits of its own fused
txt2img because both read their records from here.  Host arithmetic only; the k-diffusion wrapper is an argument."""
import collections

import torch

from .. import ops
from . import sampling

READS_ETA = ("euler_ancestral", "dpmpp_2m_sde", "dpm_2_ancestral", "dpmpp_2s_ancestral", "dpmpp_sde")     # ... and `s_noise`

# one model call and the transition after it: `stage` (sampling.STAGE_*), the sampler `step` it belongs to, whether x is that step's
# result afterwards, the `sigma` the model runs at, the update  x' = a x + m x_mid + b D + c D_old + s xi,  and that sigma's model
# scalars (c_in and t of the input, D = c_skip x + c_out * model output)
Call = collections.namedtuple("Call", "stage step ends_step sigma a m b c s c_in t c_skip c_out")


class StepPlan(tuple):
    """one Call per model call of a schedule, and what chooses the launch: `family`, `two_call` (the calls are sampling.call_plan's:
    PREDICT / CORRECT pairs) and `linear` (the records carry c_skip / c_out / s / noise: every launch but DPM++ 2M's own)"""

    def __new__(cls, calls, family, two_call, linear):
        self = super().__new__(cls, calls)
        self.family, self.two_call, self.linear = family, two_call, linear
        return self

    @property
    def noisy(self):
        """some call adds noise: the schedule needs its noise table"""
        return any(call.s != 0.0 for call in self)


def step_plan(kdm, sampler, sig, dtype, *, eta=None, s_noise=None, solver_type=None, needs_linear=False):
    """`sampler`: a name or callable of sampling.LINEAR_FAMILY / TWO_CALL_FAMILY; `sig`: the schedule on the host, final 0 included;
    `dtype`: the model's.  eta / s_noise (None: the sampler's default) reach only the families that read them, solver_type
    (None: 'midpoint') only DPM++ 2M SDE.  A linear family's calls are STAGE_FULL at the schedule's own sigmas; a two-call
    family's are sampling.call_plan's, the sigma a call's model runs at rounded to `dtype` as protocol mode's `sigma * s_in` does
    (the schedule's own already are; the update's scalars keep the unrounded value, as the samplers' host arithmetic does).
    needs_linear: the caller's launch takes full records whatever the sampler (a v-prediction model, a guidance rescale, extra
    input channels); without it DPM++ 2M keeps its own launch (c_skip = 1, c_out = -sigma, no noise)."""
    family = sampling.linear_family(sampler) or sampling.two_call_family(sampler)
    if family is None:
        raise NotImplementedError(f"no step plan for sampler {getattr(sampler, '__name__', sampler)!r} (supported: "
                                  f"{', '.join(sampling.LINEAR_FAMILY + sampling.TWO_CALL_FAMILY)})")
    args = {}
    if family in READS_ETA:
        args.update({k: v for k, v in (("eta", eta), ("s_noise", s_noise)) if v is not None})
    if family == "dpmpp_2m_sde":
        args["solver_type"] = solver_type or "midpoint"
        if args["solver_type"] not in ("midpoint", "heun"):
            raise ValueError(f"`solver_type` must be 'midpoint' or 'heun', got {args['solver_type']!r}")
    two_call = family in sampling.TWO_CALL_FAMILY
    if two_call:
        calls = [(call.stage, call.step, call.ends_step, float(torch.tensor(call.sigma, dtype=torch.float64).to(dtype))) + call.coeffs
                 for call in sampling.call_plan(family, sig, **args)]
    else:
        calls = [(sampling.STAGE_FULL, i, True, float(sig[i]), a, 0.0, b, c, s)
                 for i, (a, b, c, s) in enumerate(sampling.linear_step_coefficients(family, sig, **args))]
    plan = []
    for call in calls:
        c_in, c_out, t = kdm.step_scalars(call[3])
        plan.append(Call(*call, c_in, float(t), kdm.step_skip(call[3]), c_out))
    return StepPlan(plan, family, two_call, two_call or family != "dpmpp_2m" or bool(needs_linear))


def step_record(plan, call, guidance, rescale, noise, c_in_next, t_next, sigma_next, temb_row):
    """the STEP record of `call` (an entry of `plan`) for one row; `noise`: the row's noise, None when call.s == 0; the last four:
    what the row's next model call reads - the caller's, because the fused loop and the batcher end a schedule differently.
    The optional keys choose the launch (serving.executor.step_launch, the ops wrappers): c_skip / c_out / s / noise only on a
    `linear` plan, rescale only when > 0, stage / m only on a two-call plan."""
    rec = {"mode": ops.ROW_STEP, "sigma": call.sigma, "guidance": guidance, "a": call.a, "b": call.b, "c": call.c,
           "c_in_next": c_in_next, "t_next": t_next, "sigma_next": sigma_next, "temb_row": temb_row}
    if plan.linear:
        rec.update(c_skip=call.c_skip, c_out=call.c_out, s=call.s, noise=noise)
    if rescale > 0.0:
        rec["rescale"] = rescale
    if plan.two_call:
        rec.update(stage=call.stage, m=call.m)
    return rec
