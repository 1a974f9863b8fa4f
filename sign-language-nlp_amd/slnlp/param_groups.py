"""``optimizer__param_groups``: per-parameter-group optimizer settings, for the fused and the torch-stepped path alike.

skorch's setting is a list of ``(pattern, settings)`` pairs.  ``build`` turns it into groups the way skorch's
``_get_params_for_optimizer`` does: walk the pairs in order; ``fnmatch.fnmatch(name, pattern)`` over the parameter names not
yet taken; a pattern that matches something makes one group of those parameters (in ``named_parameters()`` order) with
``settings`` on top of the optimizer's defaults; a pattern that matches nothing makes no group; whatever is left is the LAST
group, with the defaults alone.  Nothing here needs a GPU: the same groups feed ``torch.optim.X(groups)`` on the
torch-stepped path, the segment table of the fused update kernels, the schedule's dummy optimizer and the checkpoint's
index mapping.
"""
from fnmatch import fnmatch

# per-group keys the fused update implements; any other key sends the fit to the torch-stepped path
FUSED_KEYS = frozenset(("lr", "weight_decay"))
MAX_SEGMENTS = 1024          # the library's cap (GROUPS_MAX_SEGMENTS)


class Group:
    """One optimizer param group: ``names`` (``named_parameters()`` order), ``settings`` (what the pair gave; {} for the
    remainder) and ``pattern`` (None for the remainder)."""

    def __init__(self, names, settings, pattern):
        self.names, self.settings, self.pattern = list(names), dict(settings), pattern

    def __repr__(self):
        return f"Group({self.pattern!r}, {self.settings!r}, {len(self.names)} parameters)"


def as_pairs(pairs):
    """Normalise the setting: None / empty -> []; two-element lists (YAML has no tuples) are accepted as pairs."""
    out = []
    for item in pairs or ():
        if not isinstance(item, (tuple, list)) or len(item) != 2 or not isinstance(item[0], str) or not isinstance(item[1], dict):
            raise ValueError(f"optimizer__param_groups: expected (pattern, settings) pairs, got {item!r}")
        out.append((item[0], dict(item[1])))
    return out


def build(named_shapes, pairs, defaults=None):
    """``named_shapes``: the parameter names in ``named_parameters()`` order (an iterable of names, or of (name, anything)
    pairs); ``pairs``: the setting; ``defaults``: the optimizer's defaults (only used to fill ``resolved``).  Returns the list
    of ``Group`` in optimizer order (``param_groups[0]`` first)."""
    names = [n if isinstance(n, str) else n[0] for n in named_shapes]
    taken, groups = set(), []
    for pattern, settings in as_pairs(pairs):
        hit = [n for n in names if n not in taken and fnmatch(n, pattern)]
        if hit:
            taken.update(hit)
            groups.append(Group(hit, settings, pattern))
    rest = [n for n in names if n not in taken]
    if rest:
        groups.append(Group(rest, {}, None))
    return groups


def torch_groups(groups, named_parameters):
    """The argument of ``torch.optim.X(...)``: one dict per group, ``params`` plus the group's own settings."""
    params = dict(named_parameters)
    return [{"params": [params[n] for n in g.names], **g.settings} for g in groups]


def resolved(groups, defaults, key):
    """``key`` of every group: the group's own value, else the optimizer's default."""
    return [float(g.settings.get(key, defaults[key])) for g in groups]


def fused_ok(pairs):
    """Whether every pair's settings stay within what the fused update does per group."""
    return all(set(s) <= FUSED_KEYS for _, s in as_pairs(pairs))


def positions(groups):
    """torch numbers an optimizer's ``state`` by position across the groups in group order: position -> parameter name."""
    return [n for g in groups for n in g.names]


def segments(groups, entries, total):
    """The fused update's segment table over the arena: ``entries`` [(name, shape, offset)] (offsets in floats, 16-byte
    aligned, ascending), ``total`` arena floats.  Returns (seg_begin, seg_group): segment s covers floats
    [seg_begin[s], seg_begin[s + 1]) -- the last one to ``total`` -- and belongs to group seg_group[s].  The table covers the
    arena exactly once, is sorted, and adjacent entries of one group are merged; the padding behind an entry (and an arena
    entry that is no parameter) goes with the entry before it -- no gradient ever lands there."""
    of = {n: gi for gi, g in enumerate(groups) for n in g.names}
    begin, group = [], []
    for name, _, off in sorted(entries, key=lambda e: e[2]):
        if off % 4:
            raise ValueError(f"param_groups.segments: {name} at float offset {off} is not 16-byte aligned")
        gi = of.get(name, group[-1] if group else None)
        if gi is None:
            raise ValueError(f"param_groups.segments: {name} is in no group")
        if group and group[-1] == gi:
            continue
        begin.append(0 if not begin else int(off))
        group.append(gi)
    if not begin or begin[-1] >= total:
        raise ValueError("param_groups.segments: empty table")
    if len(begin) > MAX_SEGMENTS:
        raise ValueError(f"optimizer__param_groups: {len(begin)} segments over the arena, the fused update takes at most {MAX_SEGMENTS}")
    return begin, group
