"""A stated subset of Cassandra's `.pomdp` text format (the format of the classic finite POMDPs: Tiger, Hallway, Tag),
parsed into dense numpy tables for `TabularPOMDPEnv.from_pomdp`. Pure numpy: nothing here touches the GPU.

Accepted:
    discount: <float>
    values: reward
    states: <count> | <name> <name> ...          (likewise actions: and observations:)
    start: <S probabilities> | uniform           (the probabilities on the same line or on the next ones)
    T: <a> : <s> : <s'> <prob>                    one entry
    T: <a> : <s>                                  then a row of S probabilities, or `uniform`
    T: <a>                                        then an S x S matrix, or `uniform`, or `identity`
    O: <a> : <s'> : <o> <prob>                    one entry
    O: <a> : <s'>                                 then a row of O probabilities, or `uniform`
    O: <a>                                        then an S x O matrix, or `uniform`
    R: <a> : <s> : <s'> : * <value>               the observation field must be `*` (rewards do not depend on the obs)
Every <a>, <s>, <s'>, <o> is a name, an index or `*` (all of them). `#` starts a comment. Later lines override earlier
ones. Anything else (values: cost, start: <state>, start include / exclude, the row and matrix forms of R, a reward that
names an observation, an unknown name, a wrong count of numbers) raises ValueError with the line number.
"""
import numpy as np

_SECTIONS = ("states", "actions", "observations")


class _Lines:
    """The non-empty lines without their comments, as (line number, text)."""

    def __init__(self, text):
        self.rows = []
        for n, line in enumerate(str(text).splitlines(), 1):
            line = line.split("#", 1)[0].strip()
            if line:
                self.rows.append((n, line))
        self.i = 0

    def more(self):
        return self.i < len(self.rows)

    def peek(self):
        return self.rows[self.i]

    def take(self):
        self.i += 1
        return self.rows[self.i - 1]


def _fail(n, msg):
    raise ValueError(f"line {n}: {msg}")


def _number(tok, n):
    try:
        v = float(tok)
    except ValueError:
        _fail(n, f"expected a number, got {tok!r}")
    if not np.isfinite(v):
        _fail(n, f"expected a finite number, got {tok!r}")
    return v


def _values(lines, n0, rest, count, keywords, what):
    """`count` numbers, or one of `keywords`, from the tokens after a directive's fields (`rest`) and, while they do
    not suffice, from the following lines (a line with a colon starts the next directive and is not consumed)."""
    toks = [(n0, t) for t in rest]
    while True:
        if len(toks) == 1 and toks[0][1] in keywords:
            return toks[0][1]
        if len(toks) >= count:
            break
        if not lines.more() or ":" in lines.peek()[1]:
            _fail(toks[-1][0] if toks else n0, f"{what}: expected {count} numbers or one of {sorted(keywords)}, "
                                                f"got {len(toks)} values")
        n, line = lines.take()
        toks += [(n, t) for t in line.split()]
    if len(toks) > count:
        _fail(toks[count][0], f"{what}: expected {count} numbers, got {len(toks)}")
    for n, t in toks:
        if t in ("uniform", "identity"):
            _fail(n, f"{what}: {t!r} must stand alone")
    return np.array([_number(t, n) for n, t in toks], dtype=np.float64)


def parse_pomdp(text):
    """-> dict(discount, states, actions, observations (name lists, or None where a count was given), S, A, O,
    T float64 [S, A, S], Z float64 [A, S, O], R float64 [S, A, S], start float64 [S]). Rows of T and Z that the text
    never sets stay all zero (`row_thresholds` refuses them by name). Raises ValueError naming the line."""
    lines = _Lines(text)
    names, size = {}, {}
    out = dict(discount=None)
    start = None
    T = Z = R = None

    def need_sizes(n):
        for k in _SECTIONS:
            if k not in size:
                _fail(n, f"'{k}:' must come before the first T: / O: / R: / start: line")

    def index(kind, tok, n):
        """The indices a field names: every one for `*`, else one, by name or by number."""
        if tok == "*":
            return list(range(size[kind]))
        if names[kind] is not None and tok in names[kind]:
            return [names[kind].index(tok)]
        try:
            i = int(tok)
        except ValueError:
            _fail(n, f"unknown {kind[:-1]} {tok!r}")
        if not 0 <= i < size[kind]:
            _fail(n, f"{kind[:-1]} index {i} outside [0, {size[kind]})")
        return [i]

    while lines.more():
        n, line = lines.take()
        if ":" not in line:
            _fail(n, f"expected a directive, got {line!r}")
        head, _, tail = line.partition(":")
        head = head.strip()
        if head == "discount":
            toks = tail.split()
            if len(toks) != 1:
                _fail(n, "discount: expected one number")
            out["discount"] = _number(toks[0], n)
        elif head == "values":
            if tail.split() != ["reward"]:
                _fail(n, f"values: only 'reward' is accepted, got {tail.strip()!r}")
        elif head in _SECTIONS:
            toks = tail.split()
            if T is not None or start is not None:
                _fail(n, f"'{head}:' must come before the first T: / O: / R: / start: line")
            if not toks:
                _fail(n, f"{head}: expected a count or a list of names")
            if len(toks) == 1 and toks[0].isdigit():
                names[head], size[head] = None, int(toks[0])
                if size[head] < 1:
                    _fail(n, f"{head}: expected a positive count")
            else:
                if len(set(toks)) != len(toks):
                    _fail(n, f"{head}: a name occurs twice")
                names[head], size[head] = toks, len(toks)
        elif head == "start":
            need_sizes(n)
            if ":" in tail:
                _fail(n, "start: only a probability vector or 'uniform' is accepted")
            v = _values(lines, n, tail.split(), size["states"], {"uniform"}, "start")
            start = np.full(size["states"], 1.0 / size["states"]) if isinstance(v, str) else v
        elif head in ("start include", "start exclude"):
            _fail(n, f"'{head}:' is not accepted (only a probability vector or 'uniform')")
        elif head in ("T", "O", "R"):
            need_sizes(n)
            S, A, O = size["states"], size["actions"], size["observations"]
            if T is None:
                T, Z, R = np.zeros((S, A, S)), np.zeros((A, S, O)), np.zeros((S, A, S))
            fields = [f.strip() for f in tail.split(":")]
            last = fields[-1].split()
            if not last:
                _fail(n, f"{head}: an empty field")
            fields[-1], rest = last[0], last[1:]
            if any(not f or len(f.split()) != 1 for f in fields):
                _fail(n, f"{head}: an empty or malformed field")
            acts = index("actions", fields[0], n)
            if head == "T":
                if len(fields) > 3:
                    _fail(n, "T: at most three fields (action : state : next state)")
                if len(fields) == 3:
                    v = _values(lines, n, rest, 1, set(), "T entry")
                    for s in index("states", fields[1], n):
                        for s1 in index("states", fields[2], n):
                            T[s, acts, s1] = v[0]
                elif len(fields) == 2:
                    v = _values(lines, n, rest, S, {"uniform"}, "T row")
                    row = np.full(S, 1.0 / S) if isinstance(v, str) else v
                    for s in index("states", fields[1], n):
                        T[s, acts, :] = row
                else:
                    v = _values(lines, n, rest, S * S, {"uniform", "identity"}, "T matrix")
                    mat = (np.eye(S) if v == "identity" else np.full((S, S), 1.0 / S)) if isinstance(v, str) \
                        else v.reshape(S, S)
                    for a in acts:
                        T[:, a, :] = mat
            elif head == "O":
                if len(fields) > 3:
                    _fail(n, "O: at most three fields (action : next state : observation)")
                if len(fields) == 3:
                    v = _values(lines, n, rest, 1, set(), "O entry")
                    for s1 in index("states", fields[1], n):
                        for o in index("observations", fields[2], n):
                            Z[acts, s1, o] = v[0]
                elif len(fields) == 2:
                    v = _values(lines, n, rest, O, {"uniform"}, "O row")
                    row = np.full(O, 1.0 / O) if isinstance(v, str) else v
                    for s1 in index("states", fields[1], n):
                        Z[acts, s1, :] = row
                else:
                    v = _values(lines, n, rest, S * O, {"uniform"}, "O matrix")
                    mat = np.full((S, O), 1.0 / O) if isinstance(v, str) else v.reshape(S, O)
                    for a in acts:
                        Z[a] = mat
            else:
                if len(fields) != 4:
                    _fail(n, "R: only the one-line form 'R: action : state : next state : * value' is accepted")
                if fields[3] != "*":
                    _fail(n, f"R: the observation field must be '*' (rewards do not depend on the obs), got "
                             f"{fields[3]!r}")
                v = _values(lines, n, rest, 1, set(), "R entry")
                for s in index("states", fields[1], n):
                    for s1 in index("states", fields[2], n):
                        R[s, acts, s1] = v[0]
        else:
            _fail(n, f"unknown directive {head!r}")
    end = lines.rows[-1][0] if lines.rows else 1
    for k in _SECTIONS:
        if k not in size:
            _fail(end, f"the text has no '{k}:' line")
    S, A, O = size["states"], size["actions"], size["observations"]
    if T is None:
        _fail(end, "the text has no T: / O: / R: line")
    if start is None:
        start = np.full(S, 1.0 / S)  # (Cassandra's default)
    out.update(states=names["states"], actions=names["actions"], observations=names["observations"], S=S, A=A, O=O,
               T=T, Z=Z, R=R, start=start)
    return out
