"""The recording executor of the serving host tests: the whole device-side interface of ServingBatcher without a device.  Every
call that would queue device work is logged in `events` as (method, executor name, arguments reduced to names and scalars); the
lists below keep what single tests read.  A request's 'latent' is the list of records applied to it."""
import torch

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules.serving import step_launch


def _name(r):
    return None if r is None else r.req.get("name")


class RecordingExec:
    device = torch.device("cpu")
    dtype = torch.float16
    step_keys = ("step", "sigma", "guidance", "a", "b", "c", "c_in_next", "t_next", "temb_row")      # of an applied STEP entry
    join_keys = ("c_in_next", "t_next", "sigma_next", "temb_row")                                    # ... JOIN entry (None: none)
    applied_known = False                   # append the slot's known-region record to every applied entry

    def __init__(self, name=None, events=None):
        self.name = name
        self.events = [] if events is None else events      # (two executors of a hires pair share one list)
        self.calls = []                     # (step_launch of the transition, n_src, n_dst, copies of the records, known)
        self.applied, self.noise_tables = {}, {}
        self.prepared, self.captured, self.runs, self.refreshes, self.finished = [], [], [], [], []
        self.warmed = 0

    def _event(self, method, *args):
        self.events.append((method, self.name) + args)

    @property
    def transitions(self):
        """(n_src, n_dst, records) of the transitions on DPM++ 2M's own launch"""
        return [c[1:4] for c in self.calls if c[0] == "rows"]

    @property
    def linear(self):
        """(n_src, n_dst, records) of the transitions on the linear family's launch"""
        return [c[1:4] for c in self.calls if c[0] == "linear"]

    # ---- no device work: not logged
    def bind_thread(self):
        pass

    def throttle(self):
        pass

    def ready(self, h):
        return True

    def noise_row(self, r, j):
        return ("noise", _name(r), j)

    def temb_row(self, r, j):
        return ("temb", _name(r), j)

    # ---- per request
    def _prepared(self, r, kind):
        self._event("prepare", _name(r), kind)
        self.prepared.append((kind, _name(r)))
        self.applied[id(r)] = []

    def prepare(self, r):
        self._prepared(r, "txt2img")

    def prepare_image(self, r):
        self._prepared(r, r.kind)
        if r.kind == "inpaint":
            r.known = {"image": ("image", _name(r)), "noise": ("noise", _name(r)), "mask": ("mask", _name(r))}

    def prepare_hires(self, r):
        self._prepared(r, "second")

    def prepare_noise(self, r, eta):
        self._event("noise", _name(r))
        self.noise_tables[_name(r)] = eta

    def hand_off(self, r, r2):
        self._event("hand_off", _name(r), r2.req.get("upscale_method", "bicubic"), r2.sig[0])
        return ("event", _name(r))

    def load_latent(self, r):
        self._event("load", _name(r), r.ready)

    def load_lane(self, r):
        self._event("lane", r.lane, _name(r))

    def finish(self, r):
        self._event("finish", _name(r))
        self.finished.append(_name(r))
        return r

    def finish_image(self, r):
        self._event("finish_image", _name(r), r.output_type)
        return r

    def flush_decodes(self):
        self._event("flush_decodes")
        return 0, 0

    def result(self, r, h):
        return (_name(r), self.applied[id(r)])

    # ---- per bucket
    def _ensure(self, what):
        new = what not in self.captured
        if new:
            self.captured.append(what)
        self._event("ensure", what, new)
        return new

    def ensure(self, n):
        return self._ensure(n)

    def ensure_control(self):
        return self._ensure("control")

    def ensure_decode(self):
        return int(self._ensure("decode"))

    def warm_adapter(self):
        self.warmed += 1

    def warm_control(self):
        self.warmed += 1

    def transition(self, n_src, n_dst, recs, known=None):
        assert known is None or len(known) == len(recs)
        launch = step_launch(recs, known)
        self.calls.append((launch, n_src, n_dst, [dict(rec) for rec in recs], known))
        self._event("transition", launch, n_src, n_dst, [(rec["mode"], _name(rec.get("req")), rec.get("step")) for rec in recs])
        for i, rec in enumerate(recs):
            if rec["mode"] == ops.ROW_IDLE:
                continue
            step = rec["mode"] == ops.ROW_STEP
            assert i < (n_src if step else n_dst)
            keys = self.step_keys if step else self.join_keys
            if keys is not None:
                entry = ("step" if step else "join",) + tuple(rec[k] for k in keys)
                self.applied[id(rec["req"])].append(entry + ((None if known is None else known[i],) if self.applied_known else ()))

    def refresh(self, n, members):
        self._event("refresh", n, [_name(m) for m in members])
        self.refreshes.append((n, list(members)))

    def set_adapter_gates(self, n, gates):
        self._event("set_adapter_gates", n, list(gates))

    def set_control(self, n, dst, gather, gates):
        self._event("set_control", n, dst, gather, gates)

    def run_control(self, n):
        self._event("run_control", n)

    def run(self, n):
        self._event("run", n)
        self.runs.append(n)
