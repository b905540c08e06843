"""Every load-time stage that computes or repairs the training split's depth prior on the device, for both trainers: one table in
run order, the checks of both flag surfaces as loops over it, and the two chains (NeRF++ ray samplers, MipNeRF-360 frames).  The
columns, the order and what a seventh stage touches: DESIGN.md 8.14.

Host side only, importable without torch, ctypes or any binding: a stage's module is imported by the first check or run of a
configuration that switches the stage on, its library by the run.
"""
import collections
import importlib
import types

VIEWS = 16                  # a switch whose domain is an int: 0 (off) .. 16
NAME = 'name'               # a switch whose domain is a type name: '' (off) or the folder suffix of another prior
# module:   the stage's module; flags: where its flag surface lives (the module itself unless the flags must import without ctypes)
# switch:   the flag(s) after depth_<name>_ that switch the stage on; the last one is its value, and the only one Config has
# domain:   VIEWS, NAME or the tuple of the value's choices (argparse holds the flags to them, check_switch the Config key)
# verb:     of '<switch> <verb> the depth prior of a run that trains on it: it needs ...'
# error / prefixed: the class its parameter refusals are raised under and whether (flags, Config) re-raise them as 'depth_<name>_*: ...';
#           error None: the parameters are checked by the run alone, and a Scene keeps the Config keys (depth_<name>_cfg) for it
# source:   its name as the source of a 'gnll' run's standard deviation, None: it has none to give
# computes: it computes the prior of depth_sup_type = <name> instead of reading the folder; anchor: or the alignment's anchor of that type
# replaces: its standard deviation replaces the one that went in instead of filling in where there is none
# scaled:   its args_params / scene_params take the scene's scale; line: the parameters its totals line takes after the switch
# samplers / frames: the adapters below; rows: the key of its rows in Scene.device_frames' result is 'depth_<name>_rows'
Stage = collections.namedtuple('Stage', 'name module flags switch domain verb error prefixed source computes anchor replaces scaled line '
                               'samplers frames', defaults=(None, (True, True), None, False, False, False, True, (), None, None))


# ------------------------------------------------------------------------------------------- the stages' calls, per chain
# samplers(M, c, v, prm) -> rows (host): the stage's *_samplers call.  c: the chain (args, samplers, device, want_std, target,
# load_anchors; a computed anchor travels in c.anchors); v: the switch's value; prm: args_params
def _points_samplers(M, c, v, prm):
    as_prior = c.target == 'prior'
    rows, depth = M.splat_samplers(c.samplers, c.device, c.args.depth_points_model, v, c.target, want_std=c.want_std and as_prior, **prm)
    if not as_prior:
        c.anchors = M.anchors_of(c.samplers, depth)
    return rows


def _align_samplers(M, c, v, prm):
    anchors = c.anchors if c.anchors is not None else c.load_anchors(v)
    return M.align_samplers(c.samplers, anchors, c.device, want_std=c.want_std, **prm)


# frames(M, c, v, prm) -> what the stage's *_priors call returns, on the device: (prior | None, ..., rows), the second its standard
# deviation where the stage names a source.  c: the chain (scene, idx, device, out = device_frames' dict so far; a computed anchor
# travels in c.anchor); prm: the checked parameters
def _points_frames(M, c, v, prm):
    got = M.splat_scene(c.scene, c.idx, c.device, prm)
    if c.scene.depth_points_target == 'prior':
        return got
    c.anchor = got[0]
    return (None,) + got[1:]


def _align_frames(M, c, v, prm):
    if c.anchor is None:
        import torch
        c.anchor = torch.from_numpy(c.scene.depths_anchor[c.idx]).to(c.device)
    return M.align_priors(c.out['depth_sup'], c.anchor, **prm)


def _comp_frames(M, c, v, prm):
    std_in = c.out.get('depth_std')
    if std_in is not None:
        std_in = std_in.contiguous()                                 # (a constant one is materialised)
    return M.complete_priors(c.out['depth_sup'], c.out['rgb_u8'], std_in, **prm)


# In run order.  Computed priors first: the repairs act on what they give.  Then the alignment, so that what is accumulated and checked
# across frames is metric; the accumulation before the check, which then verifies the denser prior; the completion last, so that the
# filters act on measurements and not on fills.
STAGES = (
    Stage('mvs', 'depth_mvs', 'depth_mvs_flags', ('views',), VIEWS, 'computes', 'DepthMvsError', source='mvs', computes=True,
          line=('planes',), samplers=lambda M, c, v, prm: M.sweep_samplers(c.samplers, c.device, v, want_std=c.want_std, **prm),
          frames=lambda M, c, v, prm: M.sweep_priors(c.out['rgb_u8'], M.DC.cams_from_scene(c.scene, c.idx), **prm)),
    Stage('points', 'depth_points', 'depth_points_flags', ('model', 'vis'), ('track', 'all'), 'computes', 'DepthPointsError',
          source='points', computes=True, anchor=True, samplers=_points_samplers, frames=_points_frames),
    Stage('align', 'depth_align', 'depth_align', ('anchor',), NAME, 'aligns', 'DepthAlignError', prefixed=(True, False),
          source='alignment', samplers=_align_samplers, frames=_align_frames),
    Stage('acc', 'depth_accumulate', 'depth_accumulate', ('views',), VIEWS, 'densifies', scaled=False,
          samplers=lambda M, c, v, prm: M.accumulate_samplers(c.samplers, c.device, v, **prm),
          frames=lambda M, c, v, prm: M.accumulate_priors(c.out['depth_sup'], M.cams_from_scene(c.scene, c.idx), v, **prm)),
    Stage('cons', 'depth_consistency', 'depth_consistency', ('views',), VIEWS, 'checks', source='consistency',
          samplers=lambda M, c, v, prm: M.filter_samplers(c.samplers, c.device, v, want_std=c.want_std, **prm),
          frames=lambda M, c, v, prm: M.filter_priors(c.out['depth_sup'], M.cams_from_scene(c.scene, c.idx), v, **prm)),
    Stage('comp', 'depth_complete', 'depth_complete', ('iters',), VIEWS, 'completes', 'DepthCompError', source='completion',
          replaces=True, frames=_comp_frames,
          samplers=lambda M, c, v, prm: M.complete_samplers(c.samplers, c.device, want_std=c.want_std, **prm)),
)
# mip360_train prints the totals lines in the order the stages were added to it, which is not the run order: kept, so that what a
# run prints does not change
MIP360_PRINT_ORDER = ('points', 'align', 'acc', 'cons', 'mvs', 'comp')
# ... and ddp_train_nerf's --help lists their flags in this one
FLAG_ORDER = ('cons', 'acc', 'align', 'comp', 'mvs', 'points')
BY_NAME = {st.name: st for st in STAGES}


def _module(st, flags=False):
    return importlib.import_module('.' + (st.flags if flags else st.module), __package__)


def add_flags(parser):
    """Every stage's flags on ddp_train_nerf's parser"""
    for name in FLAG_ORDER:
        _module(BY_NAME[name], flags=True).add_flags(parser)


# --------------------------------------------------------------------------------------------------- both flag surfaces
# error: what a refusal is raised as; key / bind: how the surface spells a key and a key with its value; needs: what a run that
# trains on the prior is switched on by; config: the Config dict (one switch per stage, and only a stage that computes the prior
# refuses a run without the depth loss) or parsed flags (every stage refuses it, and before it looks at depth_sup_type)
Surface = collections.namedtuple('Surface', 'error key bind needs config')
FLAGS = Surface(SystemExit, '--%s', '--%s %s', '--use_depth', False)


def _config_surface():
    from .mip360_data import ConfigError
    return Surface(ConfigError, 'Config.%s', 'Config.%s = %r', 'Config.compute_disp_metrics = True', True)


def check_switch(S, st, get, sup_type, trains):
    """(value, target) of the stage's switch on the surface S, or its refusal.  get(key): the surface's value of a key, None where it
    has none; value: falsy = off; target: 'prior' or 'anchor' of a stage that computes one and is on, else None."""
    keys = ['depth_%s_%s' % (st.name, k) for k in (st.switch[-1:] if S.config else st.switch)]
    raw = get(keys[-1])
    v = int(raw or 0) if st.domain == VIEWS else raw or ''
    if st.domain == VIEWS and not 0 <= v <= VIEWS:
        raise S.error('%s = %r: expected 0 (off) .. %d' % (S.key % keys[-1], raw, VIEWS))
    if not (v and get(keys[0])):
        return type(v)(), None
    subject = S.bind % (keys[0], v) if S.config else S.key % keys[0]
    needs = '%s %s the depth prior of a run that trains on it: it needs %s' % (subject, st.verb, S.needs)
    if not S.config and not trains:
        raise S.error(needs)
    target = None
    if st.computes:
        anchor = get('depth_align_anchor') or ''
        target = 'prior' if sup_type == st.name else 'anchor' if st.anchor and anchor == st.name else None
        if target is None and st.anchor:
            raise S.error('%s computes the prior that %s or the anchor that %s would read from disk: it needs one of them (they are %r '
                          'and %r)' % (subject, S.bind % ('depth_sup_type', st.name), S.bind % ('depth_align_anchor', st.name), sup_type, anchor))
        if target is None:
            raise S.error('%s computes the prior that %s would read from disk: it needs %s'
                          % (subject, S.bind % ('depth_sup_type', sup_type), S.bind % ('depth_sup_type', st.name)))
        if not trains:
            raise S.error(needs)
    if isinstance(st.domain, tuple) and v not in st.domain:
        raise S.error("%s = %r: expected '' (off), %s" % (S.key % keys[-1], v, ' or '.join(repr(m) for m in st.domain)))
    return v, target


def check_params(S, st, v, params, sup_type):
    """check_params() of a stage that is on, its refusal re-raised as the surface's"""
    M = _module(st)
    try:
        if st.domain == NAME:
            M.check_anchor(v, sup_type, S.key % ('depth_%s_%s' % (st.name, st.switch[-1])))
        return M.check_params(*((v,) if st.computes else ()), **params)      # (a computed prior's switch is a parameter of its call)
    except getattr(M, st.error) as e:
        prefix = S.key % ('depth_%s_*: ' % st.name) if st.prefixed[S.config] else ''
        raise S.error(prefix + str(e)) from None


def check_args(args):
    """ddp_train_nerf.validate_args' share: every stage's switch and, of a stage that is on, its parameters, or SystemExit.  Returns
    ({name: the switch's value}, {name: target})."""
    on, target = {}, {}
    for st in STAGES:
        on[st.name], target[st.name] = check_switch(FLAGS, st, lambda k: getattr(args, k, None), args.depth_sup_type, args.use_depth)
        if on[st.name] and st.error:
            check_params(FLAGS, st, on[st.name], _module(st).args_params(args), args.depth_sup_type)
    return on, target


def scene_switches(cfg):
    """Scene.__init__'s first call, before a folder is read, or ConfigError.  Returns (the attributes depth_<name>_<switch> of every
    stage and depth_<name>_target of the stages that compute one; is the prior computed, so that its folder is not read and need
    not exist; the type name of the alignment's anchor where its folder is read, '' without an alignment or with a computed anchor;
    std_source())"""
    S, on, target, attrs = _config_surface(), {}, {}, {}
    for st in STAGES:
        on[st.name], target[st.name] = check_switch(S, st, cfg.get, cfg['depth_sup_type'], cfg.get('compute_disp_metrics', True))
        attrs['depth_%s_%s' % (st.name, st.switch[-1])] = on[st.name]
        if st.computes:
            attrs['depth_%s_target' % st.name] = target[st.name]
    anchor = '' if 'anchor' in target.values() else next(on[st.name] for st in STAGES if st.domain == NAME)
    return attrs, 'prior' in target.values(), anchor, std_source(on, target)


def scene_params(scene, cfg):
    """Scene.__init__'s second call, once scene.scale exists: the checked parameters depth_<name>_prm of the stages that are on (or
    ConfigError) and the Config keys depth_<name>_cfg of the stages whose parameters the run checks"""
    S, attrs = _config_surface(), {}
    for st in STAGES:
        v = _scene_on(scene, st)
        if st.error is None:
            attrs['depth_%s_cfg' % st.name] = {k: x for k, x in cfg.items() if k.startswith('depth_%s_' % st.name)}
        elif v:
            attrs['depth_%s_prm' % st.name] = check_params(S, st, v, _module(st).scene_params(cfg, scene.scale), cfg['depth_sup_type'])
    return attrs


def _scene_on(scene, st):
    return getattr(scene, 'depth_%s_%s' % (st.name, st.switch[-1]))


def std_source(on, target):
    """The stage a 'gnll' run without a folder or a constant takes its standard deviation from: the first one in table order that is on
    and names a source, None without one.  (The ladder this replaces asked the points before the sweep; each of the two is the prior
    only under its own depth_sup_type, so both can never be, and the order between them decides nothing.)  A stage that computes the
    alignment's anchor gives the prior none; the alignment does."""
    return next((st.source for st in STAGES if on[st.name] and st.source and target[st.name] != 'anchor'), None)


# ------------------------------------------------------------------------------------------------------------ the chains
def _totals_line(st, M, rows, v, prm):
    return M.totals_line(rows, v, *(prm[k] for k in st.line))


def run_samplers(args, samplers, device, scale, want_std, load_anchors, log=None):
    """The NeRF++ chain: every stage that args switches on, in table order, on the training ray samplers (depth_sup and, with want_std,
    depth_std are rewritten in place).  load_anchors(type name) -> the training frames' samplers under the anchor's type, for an
    alignment whose anchor is not computed; log(line): called with a stage's totals line as it ends.  Returns {name: rows (host)}."""
    on, target = check_args(args)
    c = types.SimpleNamespace(args=args, samplers=samplers, device=device, want_std=want_std, load_anchors=load_anchors, anchors=None)
    done = {}
    for st in STAGES:
        if not on[st.name]:
            continue
        M = _module(st)
        prm = M.args_params(args, scale) if st.scaled else M.args_params(args)
        c.target = target[st.name]
        done[st.name] = rows = st.samplers(M, c, on[st.name], prm)
        if log is not None:
            log(_totals_line(st, M, rows, on[st.name], prm))
    return done


def run_frames(scene, idx, device, out):
    """The MipNeRF-360 chain: every stage the scene switches on, in table order, on out = Scene.device_frames' dict of the train split
    (frames idx): depth_sup is replaced, depth_std by the scene's source (Scene.depth_std_source) and by a stage that replaces
    it, and 'depth_<name>_rows' added"""
    c = types.SimpleNamespace(scene=scene, idx=idx, device=device, out=out, anchor=None)
    for st in STAGES:
        v = _scene_on(scene, st)
        if not v:
            continue
        M = _module(st)
        if st.error:
            prm = getattr(scene, 'depth_%s_prm' % st.name)
        else:
            kept = getattr(scene, 'depth_%s_cfg' % st.name)
            prm = M.scene_params(kept, scene.scale) if st.scaled else M.scene_params(kept)
        got = st.frames(M, c, v, prm)
        out['depth_%s_rows' % st.name] = got[-1]
        if got[0] is not None:
            out['depth_sup'] = got[0]
        if st.source and (scene.depth_std_source == st.source or (st.replaces and scene.depth_std_source is not None)):
            out['depth_std'] = got[1]
    return out


def totals_lines(scene, frames, order=MIP360_PRINT_ORDER):
    """The totals lines of the stages that left rows in frames = Scene.device_frames('train'), in `order`"""
    lines = []
    for st in (BY_NAME[name] for name in order):
        rows = frames.get('depth_%s_rows' % st.name)
        if rows is not None:
            lines.append(_totals_line(st, _module(st), rows.cpu().numpy(), _scene_on(scene, st), getattr(scene, 'depth_%s_prm' % st.name, {})))
    return lines
