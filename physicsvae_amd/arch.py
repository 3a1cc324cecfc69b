"""The architecture description: `Stack` (the hidden layers of one FC stack), `Arch` (the dims of PhysicsVAE's trainable
stacks and what becomes of them in a `pvae_config`) and `TENSOR_IDS` (the forward intermediates `HipEngine.read` names).
Layout queries only: nothing here needs a GPU.
"""
from . import _lib
from ._lib import ACT_KINDS, NET_MD, NET_MH, NET_PR, NET_TE, NET_WM, PRIOR_KINDS

TENSOR_IDS = {"mu": 0, "logvar": 1, "z": 2, "a_hat": 3, "s2_hat": 4, "eps": 5, "prior_mu": 6}


class Stack:
    """Hidden layers of one FC stack as `FC.__init__` accepts them (rmt:234-270): a width and an activation per
    layer ("linear" / None: none).  `gen_layers(width, depth)` (tpv:180-192) is the special case one width, one
    activation; `Stack.of((width, depth), act)` builds that."""

    def __init__(self, widths, acts="relu"):
        self.widths = tuple(int(w) for w in widths)
        if isinstance(acts, str) or acts is None:
            acts = [acts] * len(self.widths)
        self.acts = tuple("linear" if a is None else a for a in acts)
        if not self.widths or len(self.widths) > _lib.MAX_HIDDEN or min(self.widths) < 1:
            raise NotImplementedError("a stack needs 1..%d hidden layers of positive width, got %s" % (_lib.MAX_HIDDEN, self.widths))
        if len(self.acts) != len(self.widths):
            raise ValueError("one activation per hidden layer: %s vs %s" % (self.acts, self.widths))
        for a in self.acts:                      # "swish"/"silu": ray's Swish module (learnable beta), not offered
            if a not in _lib.LAYER_ACTS:
                raise NotImplementedError("hidden activation %r: the HIP path offers %s" % (a, sorted(_lib.LAYER_ACTS)))

    @classmethod
    def of(cls, spec, act="relu"):
        if isinstance(spec, Stack):
            return spec
        width, depth = spec
        return cls([width] * int(depth), act)

    def uniform(self, act):
        return len(set(self.widths)) == 1 and set(self.acts) == {act}

    def key(self):
        return (self.widths, self.acts)

    # (width, depth) of the first layer: what the uniform fields of pvae_config carry
    def __getitem__(self, i):
        return (self.widths[0], len(self.widths))[i]

    def __iter__(self):
        return iter((self.widths[0], len(self.widths)))


class Arch:
    """Dims of the trainable stacks (tpv:247-286 keys, gen_layers tpv:180-192).  `te` / `md` / `wm` / `pr`:
    (width, depth) with the one hidden activation `act` (everything the trainer can generate), or a `Stack`
    (per-layer widths and activations, what custom_model_config's *_layers can describe, rmt:462-510)."""

    def __init__(self, dim_body, dim_action, latent, te, md, wm, prior="normal_zero_mean_one_std", pr=None,
                 act="relu", te_inputs=("body", "task"), md_inputs=("body", "task"), mh=None, mh_range=0.5):
        self.Db, self.Da, self.Z = int(dim_body), int(dim_action), int(latent)
        # task_encoder_inputs / motor_decoder_inputs (rmt:470, 485): column windows of the full-width first layers
        self.te_inputs, self.md_inputs = tuple(te_inputs), tuple(md_inputs)
        for name, v in (("task_encoder_inputs", self.te_inputs), ("motor_decoder_inputs", self.md_inputs)):
            if v not in _lib.INPUT_BITS:
                raise NotImplementedError("%s = %r: a non-empty subset of ['body', 'task'], in that order" % (name, list(v)))
        if prior not in PRIOR_KINDS:
            raise NotImplementedError("Unknown latent_prior_type:%s" % (prior,))      # rmt:624-625
        self.prior = prior                       # latent_prior_type (rmt:614-635; oracle/refpath.py PRIORS)
        if act not in ACT_KINDS:                 # "swish"/"silu": ray's Swish module (learnable beta), not offered
            raise NotImplementedError("hidden activation %r: the HIP path offers %s" % (act, sorted(ACT_KINDS)))
        self.act = act                           # the trainer's "act_fn" (tpv:262): the default of every stack
        self.te, self.md, self.wm = Stack.of(te, act), Stack.of(md, act), Stack.of(wm, act)
        self.pr = Stack.of(pr, act) if pr is not None else self.te      # learned prior stack
        # the motor decoder's helper (rmt:490-498, 670-680): hidden layers `mh` (None: no helper), tanh output x mh_range
        self.mh = Stack.of(mh, act) if mh is not None else None
        self.mh_range = float(mh_range)
        if self.mh is not None and not self.mh_range > 0:
            raise AssertionError("motor_decoder_helper_range must be positive (rmt:673)")

    @property
    def te_out(self):
        return self.Z if (self.prior == "hypersphere_uniform" or self.prior is False) else 2 * self.Z   # rmt:618-623

    def config(self, max_batch, lookahead=1):
        cfg = _lib.Config(self.Db, self.Da, self.Z, self.te[0], self.te[1], self.md[0],
                          self.md[1], self.wm[0], self.wm[1], int(max_batch), int(lookahead),
                          PRIOR_KINDS[self.prior], self.pr[0], self.pr[1], ACT_KINDS[self.act])
        if self.mh is not None:
            cfg.mh_width, cfg.mh_depth, cfg.mh_range = self.mh[0], self.mh[1], self.mh_range
        for net, st in ((NET_TE, self.te), (NET_MD, self.md), (NET_WM, self.wm), (NET_PR, self.pr), (NET_MH, self.mh)):
            if st is None or st.uniform(self.act):             # (a zeroed row: the uniform stack the scalar fields describe)
                continue
            for i, (w, a) in enumerate(zip(st.widths, st.acts)):
                cfg.layer_width[net][i] = w
                cfg.layer_act[net][i] = 1 + _lib.LAYER_ACTS[a]
        cfg.te_inputs, cfg.md_inputs = _lib.INPUT_BITS[self.te_inputs], _lib.INPUT_BITS[self.md_inputs]
        return cfg

    def key(self):
        return (self.Db, self.Da, self.Z, self.te.key(), self.md.key(), self.wm.key(), self.prior, self.pr.key(), self.act,
                self.te_inputs, self.md_inputs, self.mh.key() if self.mh is not None else None, self.mh_range)
