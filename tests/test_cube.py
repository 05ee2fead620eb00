"""digital_earth_amd/cube.py without a GPU: what is written reads back value for value, a hand-written file with everything the format allows reads
as it should, and every malformed file is refused with a message that names the line."""
import numpy as np
import pytest

from digital_earth_amd import cube as cm

F = np.float32


def _write(tmp_path, text, name="t.cube"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _refused(tmp_path, text, line, word=None):
    with pytest.raises(ValueError) as e:
        cm.read_cube(_write(tmp_path, text))
    msg = str(e.value)
    assert "line %d" % line in msg, msg
    if word:
        assert word in msg, msg


@pytest.mark.parametrize("kind,n", (("3d", 2), ("3d", 5), ("1d", 2), ("1d", 300)))
def test_write_then_read_gives_the_same_cube(tmp_path, kind, n):
    rng = np.random.default_rng(n)
    table = rng.uniform(-0.5, 1.5, cm.rows(kind, n) * 3).astype(F)
    table[:4] = (0.0, 1.0, 1e-30, F(1) / F(3))
    c = cm.Cube(kind, n, table, (-0.125, 0.0, 0.1), (1.0, 2.5, 0.9), title="warm print")
    path = str(tmp_path / "a.cube")
    cm.write_cube(path, c)
    back = cm.read_cube(path)
    assert back == c and back.title == "warm print" and back.kind == kind and back.size == n
    assert (np.frombuffer(back.table, dtype=F).view(np.uint32) == table.view(np.uint32)).all()      # every float32 survives the text
    assert [F(v) for v in back.domain_min] == [F(v) for v in c.domain_min] and [F(v) for v in back.domain_max] == [F(v) for v in c.domain_max]


def test_identity_tables():
    c = cm.identity(3)
    assert c.kind == "3d" and c.size == 3 and c.domain_min == (0.0, 0.0, 0.0) and c.domain_max == (1.0, 1.0, 1.0)
    T = np.frombuffer(c.table, dtype=F).reshape(3, 3, 3, 3)
    assert tuple(T[2, 1, 0]) == (0.0, 0.5, 1.0) and tuple(T[0, 0, 1]) == (0.5, 0.0, 0.0)      # [b][g][r]: red fastest
    s = cm.identity(5, "1d")
    assert s.kind == "1d" and list(np.frombuffer(s.table, dtype=F).reshape(5, 3)[:, 1]) == [0.0, 0.25, 0.5, 0.75, 1.0]
    for bad in (1, 66):
        with pytest.raises(ValueError):
            cm.identity(bad)
    with pytest.raises(ValueError):
        cm.identity(65537, "1d")
    with pytest.raises(ValueError):
        cm.identity(4, "2d")
    assert cm.identity(65536, "1d").size == 65536 and (cm.MAX_1D, cm.MAX_3D) == (65536, 65)


def test_a_hand_written_file(tmp_path):
    text = ("# made by hand\n"
            "\n"
            "TITLE \"Day  for night\"\n"
            "   # an indented comment\n"
            "DOMAIN_MIN\t-0.5 0   0.25\n"
            "DOMAIN_MAX 1.5  1.0\t2\n"
            "\r\n"
            "LUT_3D_SIZE   2\n"
            "0 0 0\n"
            "  1.0   0.0 0.0  \n"
            "0 1 0\n"
            "1 1 0\n"
            "\n"
            "# half way\n"
            "0 0 1e0\n"
            "1 0 1\n"
            "0\t1\t1\n"
            "1.0E+00 1 .5\n"
            "\n")
    c = cm.read_cube(_write(tmp_path, text))
    assert (c.title, c.kind, c.size) == ("Day  for night", "3d", 2)
    assert c.domain_min == (-0.5, 0.0, 0.25) and c.domain_max == (1.5, 1.0, 2.0)
    assert list(c.table) == [0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0.5]
    # the scalar spelling of the domain, on a 1D and on a 3D table
    s = cm.read_cube(_write(tmp_path, "LUT_1D_SIZE 3\nLUT_1D_INPUT_RANGE 0.0 2.0\n0 0 0\n0.25 0.5 0.75\n1 1 1\n", "s.cube"))
    assert (s.kind, s.size, s.domain_min, s.domain_max) == ("1d", 3, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)) and list(s.table)[3:6] == [0.25, 0.5, 0.75]
    t = cm.read_cube(_write(tmp_path, "LUT_3D_INPUT_RANGE -1 1\nLUT_3D_SIZE 2\n" + "0.5 0.5 0.5\n" * 8, "r.cube"))
    assert t.domain_min == (-1.0,) * 3 and t.domain_max == (1.0,) * 3


def test_every_refusal_names_its_line(tmp_path):
    rows8 = "0 0 0\n" * 8
    _refused(tmp_path, "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7, 8, "7 of 8")                    # a row short: the last line read
    _refused(tmp_path, "# c\nLUT_3D_SIZE 2\n" + rows8 + "1 1 1\n", 11, "8 rows")           # a row too many
    _refused(tmp_path, "LUT_1D_SIZE 2\n0 0 0\n", 2, "1 of 2")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\n0 0\n", 3, "3 numbers")                      # a short row
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\n0 nan 0\n", 3, "finite")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\ninf 0 0\n", 3, "finite")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\n0 0 -Infinity\n", 3, "finite")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\n0 0 1e39\n", 3, "finite")                    # not a float32
    _refused(tmp_path, "LUT_3D_SIZE 2\nDOMAIN_MAX 1 inf 1\n" + rows8, 2, "finite")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 zero\n", 2, "number")
    _refused(tmp_path, "LUT_1D_SIZE 4\nLUT_3D_SIZE 2\n" + rows8, 2, "second table size")   # a shaper and a cube in one file
    _refused(tmp_path, "LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + rows8, 2, "second table size")
    _refused(tmp_path, "TITLE \"x\"\nLUT_3D_SIZE 2\nLUT_IN_VIDEO_RANGE\n" + rows8, 3, "LUT_IN_VIDEO_RANGE")      # an unknown keyword
    _refused(tmp_path, "LUT_3D_SIZE 66\n", 1, "65")                                        # beyond the library's limits
    _refused(tmp_path, "LUT_1D_SIZE 65537\n", 1, "65536")
    _refused(tmp_path, "LUT_3D_SIZE 1\n0 0 0\n", 1, "size")
    _refused(tmp_path, "LUT_3D_SIZE two\n", 1)
    _refused(tmp_path, "0 0 0\nLUT_3D_SIZE 2\n", 1, "ahead of")
    _refused(tmp_path, "LUT_3D_SIZE 2\n0 0 0\nDOMAIN_MIN 0 0 0\n", 3, "behind")
    _refused(tmp_path, "# nothing\n\n", 0)
    with pytest.raises(ValueError):                                                         # a domain that does not increase
        cm.read_cube(_write(tmp_path, "DOMAIN_MIN 0 0 1\nDOMAIN_MAX 1 1 1\nLUT_3D_SIZE 2\n" + rows8))
    for bad in (dict(table=[0.0] * 23), dict(table=[float("nan")] * 24), dict(domain_max=(1.0, 0.0, 1.0)), dict(size=1), dict(kind="4d")):
        kw = dict(kind="3d", size=2, table=[0.0] * 24)
        kw.update(bad)
        with pytest.raises(ValueError):
            cm.Cube(**kw)
