"""Every PGD_TUNE_* knob of include/pgd_amd.h is set to a value other than its default by at least one test source.

Nothing here is a hand-kept list of what is covered: the knobs are parsed from the header, their defaults from the code (the field that
pgd_tune assigns, pgdrome_amd/csrc/pgd_spmv.hip, and that field's initialiser in pgdrome_amd/csrc/pgd_internal.h), and the settings from
the syntax trees of the Python sources under tests/.  What counts as a setting of knob K to the values V:

* a call `<anything>.tune(K, V)`;
* a dictionary display whose keys are ALL knobs and whose values are integers, names or tuples / lists of them - the `{knob: value}`
  and `{knob: (value, default)}` tables the GPU tests loop over - in a module that calls `.tune` somewhere;
* a list or tuple display made of pairs `(K, V)` only - `[(3, 0), (2, 1)]`, `((TUNE_A, variant), (TUNE_B, grid_max))`, also as the
  arguments of `zip` - in a module that calls `.tune(name, name)`, i.e. loops over such pairs (in dictionaries and pairs a V given by
  name counts only beside a K given by name: small integers paired with expressions are everywhere);
* a string `"49=0"` or `"7=4,36=7"` in a module that names the PGD_TUNE environment variable.

K may be a number, a module constant (`NAME = N`, `A, B = 1, 2`), or a `TUNE_*` name of pgdrome_amd/_lib.py, plain or as an
attribute; those are resolved against the header (`TUNE_X` is `PGD_TUNE_X`), not against _lib.py.  V counts with every integer that can
reach its expression: the integers written in it, and for every name in it the integers that name can hold anywhere in the module -
assignments, `for` loops and comprehensions over displays (position by position where target and elements are tuples), parameter
defaults, the arguments of the module's own functions and classes at their call sites (by position and by keyword, through any number
of calls), and pytest.mark.parametrize lists.  Names are followed per module, not per scope: the scan may count a value that never
reaches the call at run time, it does not miss one that does.  A knob is covered when one of those integers differs from its default.

What the scan cannot see - a knob that reaches pgd_tune only inside the library or the frontend, like the `index=` argument of
Context.points_locate or settings["preconditioner"] - does not count: such a knob needs a test that names it."""
import ast
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent

# Knobs that no test has to set to another value: they decide nothing at the sizes a test can afford, or are no variants of a computation.
# At most these five; any other entry fails test_the_exemptions_are_the_five_agreed_ones.
EXEMPT = {
    26: "PCG_SMALL_ROWS: moves the two-launch form's upper limit, which acts only between 2^20 rows and that limit",
    37: "STENCIL_WG_PER_CU: changes the march length only once the launch has more tiles x marches than the whole device holds",
    15: "FAULT_ITERATION: fault injection into the sharded solve, not a variant",
    33: "FAULT_STAGE: fault injection into the sharded solve, not a variant",
    34: "FAULT_STALL_MS: fault injection into the sharded solve, not a variant",
}
ALLOWED_EXEMPT = {15, 26, 33, 34, 37}


def header_knobs():
    """{name: number} of every PGD_TUNE_* enumerator."""
    text = (ROOT / "include" / "pgd_amd.h").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(PGD_TUNE_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,/}\n]", text)}


def _c_int(expr):
    """Value of a C initialiser such as `64`, `-1`, `false`, `(int64_t)1 << 40`."""
    expr = re.sub(r"\(\s*(?:u?int\d*_t|int|long|unsigned)\s*\)", "", expr.strip())
    expr = {"false": "0", "true": "1"}.get(expr, expr)
    if not re.fullmatch(r"[-+0-9 <>()*]+", expr):
        raise ValueError(expr)
    return int(eval(expr, {"__builtins__": {}}))      # digits, shifts, products and brackets only


def code_defaults(knobs):
    """{number: default}: the field pgd_tune assigns for the knob and that field's initialiser."""
    tune = (ROOT / "pgdrome_amd" / "csrc" / "pgd_spmv.hip").read_text()
    internal = (ROOT / "pgdrome_amd" / "csrc" / "pgd_internal.h").read_text()
    inits = {}
    for m in re.finditer(r"^\s+(?:int64_t|int|bool)\s+([^;()]*(?:\([^;]*)?);", internal, re.M):
        for part in re.split(r",(?![^()]*\))", m.group(1)):
            if "=" in part and "[" not in part:
                name, value = part.split("=", 1)
                try:
                    inits.setdefault(name.strip(), _c_int(value))
                except ValueError:
                    pass
    out = {}
    for name, number in knobs.items():
        m = re.search(r"knob == %s\b[^\n]*?c->(?:comm\.)?(\w+)\s*=" % name, tune)
        assert m, "pgd_tune does not handle %s" % name
        assert m.group(1) in inits, "no initialiser found for Ctx::%s (%s)" % (m.group(1), name)
        out[number] = inits[m.group(1)]
    return out


class _Scan:
    """{knob: set of integers it is set to} of one module (see the module docstring for what counts)."""

    def __init__(self, knobs, tree, source=""):
        self.by_name = dict(knobs)
        self.by_name.update({k[4:]: v for k, v in knobs.items()})          # TUNE_X of pgdrome_amd/_lib.py
        self.numbers = set(knobs.values())
        self.tree = tree
        self.flow = {}                                                     # name -> integers it can hold
        self.defs = {}                                                     # function / class name -> parameter names (without self)
        self.found = {}
        self.consts = {}                                                   # module constants: NAME = N, A, B = 1, 2
        for stmt in tree.body:
            if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1:
                t, v = stmt.targets[0], stmt.value
                pairs = [(t, v)] if isinstance(t, ast.Name) else \
                    list(zip(t.elts, v.elts)) if isinstance(t, ast.Tuple) and isinstance(v, ast.Tuple) and len(t.elts) == len(v.elts) else []
                for tn, vn in pairs:
                    if isinstance(tn, ast.Name) and self._int(vn) is not None:
                        self.consts[tn.id] = self._int(vn)
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef):
                self.defs.setdefault(node.name, self._params(node))
            elif isinstance(node, ast.ClassDef):
                for sub in node.body:
                    if isinstance(sub, ast.FunctionDef) and sub.name == "__init__":
                        self.defs[node.name] = self._params(sub)
        for _ in range(8):                                                 # values travel through names: to a fixed point
            before = {k: set(v) for k, v in self.flow.items()}
            self._flow_pass()
            if before == self.flow:
                break
        tunes = any(isinstance(n, ast.Attribute) and n.attr == "tune" for n in ast.walk(tree))
        pair_loops = any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "tune" and len(n.args) == 2 and
                         all(isinstance(a, ast.Name) and self._knob(a) is None for a in n.args) for n in ast.walk(tree))
        for node in ast.walk(tree):
            if isinstance(node, ast.Call):
                self._tune_call(node)
                if pair_loops and isinstance(node.func, ast.Name) and node.func.id == "zip" and len(node.args) == 2:
                    self._zip(node)
            elif isinstance(node, ast.Dict) and tunes:
                self._dict(node)
            elif pair_loops and isinstance(node, (ast.List, ast.Tuple)):
                self._pairs(node)
            elif isinstance(node, ast.Constant) and isinstance(node.value, str) and "PGD_TUNE" in source:
                if re.fullmatch(r"\d+=-?\d+(,\d+=-?\d+)*", node.value):
                    for item in node.value.split(","):
                        k, v = map(int, item.split("="))
                        if k in self.numbers:
                            self.found.setdefault(k, set()).add(v)

    @staticmethod
    def _params(fn):
        names = [a.arg for a in fn.args.posonlyargs + fn.args.args]
        return names[1:] if names[:1] in (["self"], ["cls"]) else names

    # ---- what an expression can be
    def _int(self, node):
        """The integer a knob or constant expression stands for, None if it is not one."""
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            n = self._int(node.operand)
            return None if n is None else -n
        if isinstance(node, ast.Name):
            return self.by_name.get(node.id, self.consts.get(node.id))
        if isinstance(node, ast.Attribute):
            return self.by_name.get(node.attr)
        return None

    def _knob(self, node):
        n = self._int(node)
        return n if n in self.numbers else None

    def _values(self, node):
        """Every integer that can reach the expression."""
        out = set()
        for sub in ast.walk(node):
            if isinstance(sub, ast.Constant) and type(sub.value) is int:
                out.add(sub.value)
            elif isinstance(sub, ast.UnaryOp) and isinstance(sub.op, ast.USub) and self._int(sub) is not None:
                out.add(self._int(sub))
            elif isinstance(sub, ast.Name):
                out |= self.flow.get(sub.id, set())
                if sub.id in self.by_name:
                    out.add(self.by_name[sub.id])
            elif isinstance(sub, ast.Attribute):
                out |= self.flow.get(sub.attr, set())
        return out

    # ---- how integers reach names
    def _bind(self, target, value):
        """target = value, position by position where both are displays."""
        if isinstance(target, (ast.Tuple, ast.List)):
            if isinstance(value, (ast.Tuple, ast.List)) and len(value.elts) == len(target.elts) and \
                    not any(isinstance(e, ast.Starred) for e in list(target.elts) + list(value.elts)):
                for t, v in zip(target.elts, value.elts):
                    self._bind(t, v)
            else:
                for t in target.elts:
                    self._bind(t.value if isinstance(t, ast.Starred) else t, value)
        elif isinstance(target, ast.Name):
            self.flow.setdefault(target.id, set()).update(self._values(value))
        elif isinstance(target, ast.Attribute):
            self.flow.setdefault(target.attr, set()).update(self._values(value))

    def _bind_each(self, target, iterable):
        """for target in iterable."""
        if isinstance(iterable, ast.Call) and isinstance(iterable.func, ast.Name) and iterable.func.id == "zip" and \
                isinstance(target, (ast.Tuple, ast.List)) and len(target.elts) == len(iterable.args):
            for t, seq in zip(target.elts, iterable.args):
                self._bind_each(t, seq)
        elif isinstance(iterable, (ast.Tuple, ast.List)):
            for e in iterable.elts:
                self._bind(target, e)
        else:
            self._bind(target, iterable)

    def _flow_pass(self):
        for node in ast.walk(self.tree):
            if isinstance(node, ast.Assign):
                for t in node.targets:
                    self._bind(t, node.value)
            elif isinstance(node, (ast.For, ast.comprehension)):
                self._bind_each(node.target, node.iter)
            elif isinstance(node, ast.FunctionDef):
                args = node.args.posonlyargs + node.args.args
                for a, d in zip(args[len(args) - len(node.args.defaults):], node.args.defaults):
                    self.flow.setdefault(a.arg, set()).update(self._values(d))
                for a, d in zip(node.args.kwonlyargs, node.args.kw_defaults):
                    if d is not None:
                        self.flow.setdefault(a.arg, set()).update(self._values(d))
                for dec in node.decorator_list:
                    self._parametrize(dec)
            elif isinstance(node, ast.Call):
                name = node.func.id if isinstance(node.func, ast.Name) else node.func.attr if isinstance(node.func, ast.Attribute) else None
                params = self.defs.get(name, [])
                for i, a in enumerate(node.args):
                    if isinstance(a, ast.Starred):
                        for p in params[i:]:
                            self.flow.setdefault(p, set()).update(self._values(a.value))
                        break
                    if i < len(params):
                        self.flow.setdefault(params[i], set()).update(self._values(a))
                if name in self.defs:
                    for kw in node.keywords:
                        if kw.arg:
                            self.flow.setdefault(kw.arg, set()).update(self._values(kw.value))

    def _parametrize(self, dec):
        if not (isinstance(dec, ast.Call) and isinstance(dec.func, ast.Attribute) and dec.func.attr == "parametrize" and len(dec.args) >= 2):
            return
        names, cases = dec.args[0], dec.args[1]
        if not (isinstance(names, ast.Constant) and isinstance(names.value, str)):
            return
        names = [n.strip() for n in names.value.split(",")]
        target = ast.Name(id=names[0]) if len(names) == 1 else ast.Tuple(elts=[ast.Name(id=n) for n in names])
        self._bind_each(target, cases)

    # ---- the settings
    def _tune_call(self, node):
        if isinstance(node.func, ast.Attribute) and node.func.attr == "tune" and len(node.args) == 2:
            k = self._knob(node.args[0])
            if k is not None:
                self.found.setdefault(k, set()).update(self._values(node.args[1]))

    def _dict(self, node):
        keys = [None if k is None else self._knob(k) for k in node.keys]
        if keys and None not in keys:
            named = any(isinstance(k, (ast.Name, ast.Attribute)) for k in node.keys)      # values by name only beside a key by name
            vals = []
            for v in node.values:
                elts = v.elts if isinstance(v, (ast.Tuple, ast.List)) else [v]
                ok = all(self._int(e) is not None or (named and isinstance(e, (ast.Name, ast.Attribute))) for e in elts)
                vals.append(self._values(v) if ok and elts else None)
            if None not in vals:
                for k, vs in zip(keys, vals):
                    self.found.setdefault(k, set()).update(vs)

    def _pairs(self, node):
        elts = node.elts
        named = any(isinstance(e, ast.Tuple) and e.elts and isinstance(e.elts[0], (ast.Name, ast.Attribute)) for e in elts)
        if elts and all(isinstance(e, ast.Tuple) and len(e.elts) == 2 and self._knob(e.elts[0]) is not None and
                        (self._int(e.elts[1]) is not None or (named and isinstance(e.elts[1], (ast.Name, ast.Attribute)))) for e in elts):
            for e in elts:
                self.found.setdefault(self._knob(e.elts[0]), set()).update(self._values(e.elts[1]))

    def _zip(self, node):
        ks, vs = node.args
        if isinstance(ks, (ast.Tuple, ast.List)) and ks.elts and all(self._knob(e) is not None for e in ks.elts) and \
                any(isinstance(e, (ast.Name, ast.Attribute)) for e in ks.elts):
            if isinstance(vs, (ast.Tuple, ast.List)) and len(vs.elts) == len(ks.elts):
                for k, v in zip(ks.elts, vs.elts):
                    self.found.setdefault(self._knob(k), set()).update(self._values(v))
            else:
                for k in ks.elts:
                    self.found.setdefault(self._knob(k), set()).update(self._values(vs))


def settings_in_tests(knobs):
    """{knob: {value: [files]}} over every Python source under tests/ but this one."""
    out = {}
    for path in sorted((ROOT / "tests").rglob("*.py")):
        if path.resolve() == pathlib.Path(__file__).resolve():
            continue
        text = path.read_text()
        scan = _Scan(knobs, ast.parse(text, filename=str(path)), text)
        for k, vals in scan.found.items():
            for v in vals:
                out.setdefault(k, {}).setdefault(v, []).append(path.name)
    return out


def test_the_header_and_the_code_agree_on_the_knobs():
    knobs = header_knobs()
    assert len(knobs) >= 70 and len(set(knobs.values())) == len(knobs)
    defaults = code_defaults(knobs)
    assert set(defaults) == set(knobs.values())
    # a few the header states in words
    assert defaults[knobs["PGD_TUNE_SPMV_ROWS"]] == 64 and defaults[knobs["PGD_TUNE_SPMV_FETCH_DEPTH"]] == 6
    assert defaults[knobs["PGD_TUNE_FAULT_ITERATION"]] == -1 and defaults[knobs["PGD_TUNE_HALO_OVERLAP_MIN_ROWS"]] == 1 << 40
    assert defaults[knobs["PGD_TUNE_COMM_SELF_PERIODIC"]] == 0 and defaults[knobs["PGD_TUNE_PCG_SMALL_ROWS"]] == 1 << 22


def test_the_scan_resolves_constants_dicts_loops_calls_and_pairs():
    knobs = header_knobs()
    src = (
        "import pytest\n"
        "from pgdrome_amd import _lib\n"
        "FORCE, DEPTH, FETCH = 7, 38, 24\n"
        "ROWS = 48\n"
        "TABLE = {'a': {FORCE: 4, DEPTH: 6}, 'b': {25: (0, 1)}}\n"
        "MADE = [{FETCH: fetch} for fetch in (3, 6)]\n"
        "BY_NUMBER = [{21: length} for length in (5, 12)]\n"
        "NOT_KNOBS = {7: 4, 1000: 1}\n"
        "FLOATS = {3: 0.5}\n"
        "def f(ctx):\n"
        "    for rows in (2, 4):\n"
        "        ctx.tune(ROWS, rows)\n"
        "    ctx.tune(_lib.TUNE_GRAM_VARIANT, 0)\n"
        "    ctx.tune(1000, 5)\n"
        "    ctx.tune(13, unknown)\n"
        "    for name, storage in (('vectors', 0), ('block', 2)):\n"
        "        ctx.tune(_lib.TUNE_BLOCK_STORAGE, storage)\n"
        "def solves(ctx, k55, k56=1):\n"
        "    ctx.tune(55, k55)\n"
        "    ctx.tune(56, k56)\n"
        "class Knobs:\n"
        "    def __init__(self, ctx, variant=1, grid_max=0):\n"
        "        self.ctx, self.values = ctx, (variant, grid_max)\n"
        "    def set(self, variant, grid_max):\n"
        "        for knob, val in ((_lib.TUNE_POST_VARIANT, variant), (_lib.TUNE_POST_GRID_MAX, grid_max)):\n"
        "            self.ctx.tune(knob, val)\n"
        "    def __enter__(self):\n"
        "        self.set(*self.values)\n"
        "@pytest.mark.parametrize('variant,cap', [(0, 3), (1, 5)])\n"
        "def test_a(ctx, variant, cap):\n"
        "    solves(ctx, 1, k56=0)\n"
        "    with Knobs(ctx, variant, cap):\n"
        "        pass\n"
        "    for k, v in [(6, 0), (47, 1)]:\n"
        "        ctx.tune(k, v)\n"
        "    shape = (1, 0)\n"
        "    monkeypatch.setenv('PGD_TUNE', '49=0')\n"
    )
    found = _Scan(knobs, ast.parse(src), src).found
    # (names are followed per module and `*self.values` reaches every parameter of `set`: knobs 70 and 71 see the values of both)
    assert found == {7: {4}, 38: {6}, 25: {0, 1}, 24: {3, 6}, 48: {2, 4}, 62: {0}, 13: set(), 54: {0, 2}, 55: {1}, 56: {0, 1},
                     70: {0, 1, 3, 5}, 71: {0, 1, 3, 5}, 6: {0}, 47: {1}, 49: {0}}, found


def test_the_exemptions_are_the_five_agreed_ones():
    assert set(EXEMPT) <= ALLOWED_EXEMPT and len(EXEMPT) <= 5
    assert all(isinstance(r, str) and r and "\n" not in r for r in EXEMPT.values())


def test_every_knob_is_set_to_a_value_other_than_its_default_by_some_test():
    knobs = header_knobs()
    defaults = code_defaults(knobs)
    seen = settings_in_tests(knobs)
    missing = []
    for name, number in sorted(knobs.items(), key=lambda kv: kv[1]):
        others = {v: f for v, f in seen.get(number, {}).items() if v != defaults[number]}
        print("%-34s %3d default %-14d %s" % (name, number, defaults[number],
                                              ", ".join("%d (%s)" % (v, f[0]) for v, f in sorted(others.items())[:4]) or "-"))
        if not others and number not in EXEMPT:
            missing.append((name, number, defaults[number]))
    assert not missing, "no test sets these knobs to a value other than the default: %s" % missing
