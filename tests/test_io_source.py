"""The ``.source`` deck reader and writer (ibamr_amd.io.read_source / write_source) and the
host-side SourceSpecs: a round trip, every error IBStandardInitializer::readSourceFiles
raises, the map semantics of a vertex listed twice, and the running source offset.  No GPU.
"""
import numpy as np
import pytest

from ibamr_amd import io


def write(tmp_path, text, name="s.source"):
    p = tmp_path / name
    p.write_text(text)
    return p


GOOD = """2   # two sources
  inlet valve  ! trailing comment
outlet
1.5e-1
0.25   % a radius
3
0 1
4 0
2 1
"""


def test_read_source_format(tmp_path):
    d = io.read_source(write(tmp_path, GOOD), 5)
    assert d.names == ["inlet valve", "outlet"]
    assert d.radii.tolist() == [0.15, 0.25]
    assert d.node.tolist() == [0, 2, 4] and d.source.tolist() == [1, 1, 0]
    assert d.node.dtype == np.int32 and d.source.dtype == np.int32 and d.radii.dtype == np.float64
    d = io.read_source(write(tmp_path, GOOD), 5, vertex_offset=10, source_offset=3)
    assert d.node.tolist() == [10, 12, 14] and d.source.tolist() == [4, 4, 3]


def test_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    names = ["a", "b c", "d"]
    radii = rng.uniform(0.01, 0.3, 3)
    node = rng.permutation(40)[:17]
    source = rng.integers(0, 3, 17)
    p = tmp_path / "rt.source"
    io.write_source(p, names, radii, node, source)
    d = io.read_source(p, 40)
    assert d.names == names
    assert np.array_equal(d.radii.view(np.int64), radii.view(np.int64))  # bit for bit
    o = np.argsort(node)
    assert np.array_equal(d.node, node[o]) and np.array_equal(d.source, source[o])
    # written again from what was read, the file is the same
    q = tmp_path / "rt2.source"
    io.write_source(q, d.names, d.radii, d.node, d.source)
    assert io.read_source(q, 40).node.tolist() == d.node.tolist()


def test_vertex_listed_twice_keeps_its_last_source(tmp_path):
    d = io.read_source(write(tmp_path, "2\na\nb\n0.1\n0.1\n3\n1 0\n2 1\n1 1\n"), 4)
    assert d.node.tolist() == [1, 2] and d.source.tolist() == [1, 1]


@pytest.mark.parametrize("text, line, detail", [
    ("", 1, "Premature end"),
    ("x\n", 1, "Invalid entry"),
    ("0\n", 1, "Invalid entry"),
    ("-2\n", 1, "Invalid entry"),
    ("2\na\n", 3, "Premature end"),
    ("2\na\nb\n0.1\n", 5, "Premature end"),
    ("2\na\nb\n0.1\nzero\n", 5, "Invalid entry"),
    ("2\na\nb\n0.1\n0.0\n", 5, "Invalid entry"),
    ("2\na\nb\n-0.1\n0.2\n", 4, "Invalid entry"),
    ("2\na\nb\n0.1\n0.2\n", 6, "Premature end"),
    ("2\na\nb\n0.1\n0.2\n0\n", 6, "Invalid entry"),
    ("2\na\nb\n0.1\n0.2\n2\n0 0\n", 8, "Premature end"),
    ("2\na\nb\n0.1\n0.2\n2\n0 0\nq 1\n", 8, "Invalid entry"),
    ("2\na\nb\n0.1\n0.2\n2\n0 0\n5 1\n", 8, "vertex index 5 is out of range"),
    ("2\na\nb\n0.1\n0.2\n2\n0 0\n-1 1\n", 8, "vertex index -1 is out of range"),
    ("2\na\nb\n0.1\n0.2\n2\n0 0\n1\n", 8, "Invalid entry"),
    ("2\na\nb\n0.1\n0.2\n2\n0 2\n1 1\n", 7, "meter index 2 is out of range"),
    ("2\na\nb\n0.1\n0.2\n2\n0 -1\n1 1\n", 7, "meter index -1 is out of range"),
])
def test_errors_name_the_line(tmp_path, text, line, detail):
    p = write(tmp_path, text)
    with pytest.raises(ValueError) as e:
        io.read_source(p, 5)
    msg = str(e.value)
    assert detail in msg and f"line {line} of file {p}" in msg, msg


def test_missing_file_and_writer_arguments(tmp_path):
    with pytest.raises(FileNotFoundError):
        io.read_source(tmp_path / "none.source", 3)
    with pytest.raises(ValueError):
        io.write_source(tmp_path / "w.source", ["a"], [0.1, 0.2], [0], [0])
    with pytest.raises(ValueError):
        io.write_source(tmp_path / "w.source", ["a # b"], [0.1], [0], [0])
    with pytest.raises(ValueError):
        io.write_source(tmp_path / "w.source", ["a"], [0.1], [], [])


def test_source_specs_from_decks_and_renumbering(tmp_path):
    from ibamr_amd.sources import SourceSpecs
    io.write_source(tmp_path / "a.source", ["a0", "a1"], [0.1, 0.2], [0, 3, 2], [1, 0, 1])
    io.write_source(tmp_path / "b.source", ["b0"], [0.3], [1, 0], [0, 0])
    da = io.read_source(tmp_path / "a.source", 4)
    db = io.read_source(tmp_path / "b.source", 3, vertex_offset=4, source_offset=2)
    s = SourceSpecs.from_deck(da, db, num_vertex=7)
    assert s.names == ["a0", "a1", "b0"] and s.radii.tolist() == [0.1, 0.2, 0.3] and s.num_source == 3
    assert s.node.tolist() == [0, 2, 3, 4, 5] and s.source.tolist() == [1, 1, 0, 2, 2]
    with pytest.raises(ValueError):  # the second deck read without its source offset
        SourceSpecs.from_deck(da, io.read_source(tmp_path / "b.source", 3, vertex_offset=4), num_vertex=7)
    a = s.arrays()
    assert a.node.tolist() == s.node.tolist() and a.source.tolist() == s.source.tolist()
    perm = np.array([6, 5, 4, 3, 2, 1, 0])
    a = s.arrays(perm)
    assert a.node.tolist() == [1, 2, 3, 4, 6] and a.source.tolist() == [2, 2, 0, 1, 1]
    assert a.node.dtype == np.int32 and a.source.dtype == np.int32
    with pytest.raises(ValueError):
        s.arrays(perm[:3])
    with pytest.raises(ValueError):
        SourceSpecs(["a"], [0.1], [0, 0], [0, 0])   # a node named twice
    with pytest.raises(ValueError):
        SourceSpecs(["a"], [-0.1], [0], [0])
    with pytest.raises(ValueError):
        SourceSpecs(["a"], [0.1], [0], [1])
