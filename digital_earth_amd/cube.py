"""A reader and writer for .cube lookup tables, the exchange format of looks, print emulations and display calibrations — what Renderer.set_look()
loads (include/digital_earth_look.h): pure Python, no dependency.

    look = read_cube("print_emulation.cube")        # a Cube: title, kind "1d" or "3d", size, domain_min, domain_max, table
    write_cube("identity33.cube", identity(33))

The format is Adobe's Cube LUT Specification 1.0: text, one statement per line, `#` starts a comment line, blank lines and any run of blanks or
tabs are allowed.  Keywords ahead of the data: TITLE "text"; DOMAIN_MIN r g b and DOMAIN_MAX r g b (default 0 0 0 and 1 1 1); LUT_1D_SIZE n or
LUT_3D_SIZE n, exactly one of the two.  Also read: the scalar spelling LUT_1D_INPUT_RANGE lo hi / LUT_3D_INPUT_RANGE lo hi that other tools
write for the same domain on all three channels.  Then n (1D) or n^3 (3D) rows of three numbers; in a 3D table red changes fastest, and the
table is kept in that order: entry (r, g, b) at ((b n + g) n + r) 3 + c.  Everything that is wrong is refused with a ValueError that names the line.

Not read: Resolve's files that hold a shaper AND a cube (both sizes in one file: refused), .3dl, CLF, ICC."""
import math
from array import array

MAX_1D = 65536      # DE_LOOK_MAX_1D
MAX_3D = 65         # DE_LOOK_MAX_3D
KINDS = ("1d", "3d")
_F32_MAX = 3.4028234663852886e38


class Cube:
    """One table.  kind "1d": size rows, three curves; kind "3d": size^3 rows, red fastest.  table: array('f') of rows x 3 values in file order;
    domain_min, domain_max: 3-tuples of floats, the inputs that the first and the last entry of each axis stand for."""
    __slots__ = ("title", "kind", "size", "domain_min", "domain_max", "table")

    def __init__(self, kind, size, table, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0), title=""):
        if kind not in KINDS:
            raise ValueError("kind must be '1d' or '3d'")
        size = int(size)
        _check_size(kind, size, "")
        if hasattr(table, "ravel") and hasattr(table, "astype"):      # a numpy array of any shape, in C order (numpy itself is not needed here)
            table = array("f", table.ravel().astype("float32").tobytes())
        elif not (isinstance(table, array) and table.typecode == "f"):
            table = array("f", table)
        if len(table) != rows(kind, size) * 3:
            raise ValueError("a %s table of size %d has %d values, not %d" % (kind, size, rows(kind, size) * 3, len(table)))
        self.domain_min, self.domain_max = tuple(float(v) for v in domain_min), tuple(float(v) for v in domain_max)
        if len(self.domain_min) != 3 or len(self.domain_max) != 3:
            raise ValueError("domain_min and domain_max have three values each")
        _check_domain(self.domain_min, self.domain_max, "")
        if not all(math.isfinite(v) for v in table):
            raise ValueError("a table value is not finite")
        self.title, self.kind, self.size, self.table = str(title), kind, size, table

    def __eq__(self, other):
        return isinstance(other, Cube) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __repr__(self):
        return "Cube(%r, %d, title=%r, domain_min=%r, domain_max=%r)" % (self.kind, self.size, self.title, self.domain_min, self.domain_max)


def rows(kind, size):
    return size if kind == "1d" else size ** 3


def _check_size(kind, size, where):
    top = MAX_1D if kind == "1d" else MAX_3D
    if size < 2 or size > top:
        raise ValueError("%sa %s table has a size of 2 ... %d, not %d" % (where, kind, top, size))


def _check_domain(lo, hi, where):
    if not all(math.isfinite(v) for v in lo + hi):
        raise ValueError("%sthe domain is not finite" % where)
    if not all(b > a for a, b in zip(lo, hi)):
        raise ValueError("%sDOMAIN_MAX must be above DOMAIN_MIN in every channel" % where)


def identity(n, kind="3d"):
    """The table that changes nothing: entry i of an axis is i / (n - 1)."""
    n = int(n)
    if kind not in KINDS:
        raise ValueError("kind must be '1d' or '3d'")
    _check_size(kind, n, "")
    ramp = [i / (n - 1) for i in range(n)]
    t = array("f")
    if kind == "1d":
        for v in ramp:
            t.extend((v, v, v))
    else:
        for b in ramp:
            for g in ramp:
                for r in ramp:
                    t.extend((r, g, b))
    return Cube(kind, n, t, title="identity")


def _numbers(words, count, where):
    if len(words) != count:
        raise ValueError("%sexpected %d numbers, found %d" % (where, count, len(words)))
    try:
        vals = [float(w) for w in words]
    except ValueError:
        raise ValueError("%snot a number: %r" % (where, " ".join(words)))
    if not all(abs(v) <= _F32_MAX for v in vals):      # NaN fails too
        raise ValueError("%sa value is not finite (as a float32)" % where)
    return vals


def read_cube(path):
    """Read a .cube file into a Cube.  ValueError, naming the line, for: a wrong row count, a non-finite or unreadable number, both LUT_1D_SIZE and
    LUT_3D_SIZE in one file, an unknown keyword, a size beyond 65536 (1D) or 65 (3D), a domain that is not increasing."""
    title, kind, size = "", None, 0
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    table = array("f")
    want = 0
    last = 0
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for number, raw in enumerate(f, 1):
            line = raw.strip()
            if line.startswith("\ufeff"):
                line = line[1:].strip()
            if not line or line.startswith("#"):
                continue
            last = number
            where = "%s, line %d: " % (path, number)
            words = line.split()
            head = words[0]
            if head[0].isalpha() or head[0] == "_":
                key = head.upper()
                if key in ("NAN", "INF", "INFINITY"):
                    raise ValueError("%sa value is not finite" % where)
                if len(table):
                    raise ValueError("%skeyword %s behind the first row of the table" % (where, head))
                if key == "TITLE":
                    rest = line[len(head):].strip()
                    title = rest[1:-1] if len(rest) >= 2 and rest[0] == '"' and rest[-1] == '"' else rest
                elif key == "DOMAIN_MIN":
                    lo = tuple(_numbers(words[1:], 3, where))
                elif key == "DOMAIN_MAX":
                    hi = tuple(_numbers(words[1:], 3, where))
                elif key in ("LUT_1D_INPUT_RANGE", "LUT_3D_INPUT_RANGE"):
                    a, b = _numbers(words[1:], 2, where)
                    lo, hi = (a, a, a), (b, b, b)
                elif key in ("LUT_1D_SIZE", "LUT_3D_SIZE"):
                    if kind is not None:
                        raise ValueError("%sa second table size: a file holds one 1D or one 3D table (a shaper and a cube in one file are not read)" % where)
                    if len(words) != 2 or not words[1].isdigit():
                        raise ValueError("%s%s takes one whole number" % (where, head))
                    kind, size = ("1d" if key == "LUT_1D_SIZE" else "3d"), int(words[1])
                    _check_size(kind, size, where)
                    want = rows(kind, size)
                else:
                    raise ValueError("%sunknown keyword %s" % (where, head))
                continue
            if kind is None:
                raise ValueError("%sa table row ahead of LUT_1D_SIZE / LUT_3D_SIZE" % where)
            if len(table) >= want * 3:
                raise ValueError("%srow %d of a table that has %d rows" % (where, want + 1, want))
            table.extend(_numbers(words, 3, where))
    if kind is None:
        raise ValueError("%s, line %d: the file ends without LUT_1D_SIZE or LUT_3D_SIZE" % (path, last))
    if len(table) != want * 3:
        raise ValueError("%s, line %d: the file ends after %d of %d rows" % (path, last, len(table) // 3, want))
    _check_domain(lo, hi, "%s: " % path)
    return Cube(kind, size, table, lo, hi, title)


def write_cube(path, cube):
    """Write a Cube as a .cube file that read_cube() gives back value for value (nine significant digits: every float32 survives)."""
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        if cube.title:
            f.write('TITLE "%s"\n' % cube.title.replace('"', "'"))
        f.write("LUT_%s_SIZE %d\n" % (cube.kind.upper(), cube.size))
        f.write("DOMAIN_MIN %s\n" % " ".join("%.9g" % v for v in cube.domain_min))
        f.write("DOMAIN_MAX %s\n" % " ".join("%.9g" % v for v in cube.domain_max))
        t = cube.table
        f.writelines("%.9g %.9g %.9g\n" % (t[i], t[i + 1], t[i + 2]) for i in range(0, len(t), 3))
