"""The table of tests/golden/make_golden.py against the fixtures in that directory: every .npz has exactly one row that
writes it, every row's inputs come from earlier rows, and every generator imports without the reference."""
import glob
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402

KEPT = {'legacy_scan.npz'}     # the reference's own data, kept unchanged: no row writes it


def test_every_fixture_has_exactly_one_writer():
    written = [name for r in mg.TABLE for name in r.writes]
    assert len(written) == len(set(written))
    present = {os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, '*.npz'))}
    assert KEPT <= present and not KEPT & set(written)
    assert set(written) == present - KEPT


def test_rows_read_what_earlier_rows_write():
    assert len(mg.ROWS) == len(mg.TABLE)
    seen = set()
    for r in mg.TABLE:
        assert set(r.reads) <= seen, r.name
        seen |= set(r.writes)
    assert all(set(r.host_dependent) == set() or r.note for r in mg.TABLE)


def test_generators_import_without_the_reference(monkeypatch, tmp_path):
    monkeypatch.setenv(mg.reference.ROOT_ENV, str(tmp_path / 'absent'))
    before = set(sys.modules)
    for r in mg.TABLE:
        assert callable(mg.resolve(r)), r.name
    loaded = [m for m in set(sys.modules) - before if m.startswith(('ref_', 'f110_gym'))]
    assert not loaded, loaded
