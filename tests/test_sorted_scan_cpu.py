"""CPU tests of the two helpers every indexed scan of the cloud and mesh tools goes through (mast3r_slam/tsdf/
mesh_index.py): _index_ops, the operands of an index, and _sorted_scan, "sort the queries by Morton key, launch, scatter
the outputs back".  A stub index with a fixed permutation stands in for the Morton sort, on CPU tensors."""
import pytest
import torch

from mast3r_slam.tsdf.mesh_index import _index_ops, _sorted_scan

OUTPUTS = ((torch.float64, ()), (torch.int32, (3,)))


class StubIndex:
    def __init__(self, perm):
        self.perm, self.calls = torch.as_tensor(perm, dtype=torch.int64), 0

    def query_order(self, points):
        self.calls += 1
        assert len(points) == len(self.perm)
        return self.perm


def _queries(n):
    return torch.arange(3 * n, dtype=torch.float32).reshape(n, 3) * 0.5 + 1.0


def _scan(seen):
    """A scan whose outputs are functions of the query alone, and which records what it was given."""
    def scan(q, extra, tag, a, b):
        seen.append((q.clone(), extra, tag))
        assert q.is_contiguous() and (extra is None or extra.is_contiguous())
        a.copy_(q.double().sum(1))
        b.copy_((q * 2.0).to(torch.int32))
    return scan


def test_index_ops_without_an_index():
    assert _index_ops(None) == (0, 0, 0, 1)
    assert _index_ops(None, levels=1) == (0, 0, 0, 1)


def test_outputs_come_back_in_query_order():
    n = 7
    q, extra = _queries(n), torch.arange(n, dtype=torch.int32) * 10
    ix, seen = StubIndex([3, 0, 6, 1, 5, 2, 4]), []
    a, b = _sorted_scan(q, ix, True, OUTPUTS, _scan(seen), (extra, None))
    assert ix.calls == 1 and len(seen) == 1
    got_q, got_extra, got_none = seen[0]
    # the callback saw the queries and the per-query tensor in the index's order; None stays None
    assert torch.equal(got_q, q[ix.perm]) and torch.equal(got_extra, extra[ix.perm]) and got_none is None
    # the outputs are those of the queries as given
    assert a.dtype == torch.float64 and tuple(a.shape) == (n,) and torch.equal(a, q.double().sum(1))
    assert b.dtype == torch.int32 and tuple(b.shape) == (n, 3) and torch.equal(b, (q * 2.0).to(torch.int32))


@pytest.mark.parametrize("n, sort_queries, with_index", [(0, True, True), (1, True, True), (7, False, True),
                                                         (7, True, False)])
def test_queries_as_given(n, sort_queries, with_index):
    q, extra = _queries(n), torch.arange(n, dtype=torch.int32)
    ix, seen = StubIndex(list(reversed(range(n)))), []
    a, b = _sorted_scan(q, ix if with_index else None, sort_queries, OUTPUTS, _scan(seen), (extra, None))
    assert ix.calls == 0 and len(seen) == 1
    assert torch.equal(seen[0][0], q) and seen[0][1] is extra and seen[0][2] is None
    assert tuple(a.shape) == (n,) and tuple(b.shape) == (n, 3)
    assert torch.equal(a, q.double().sum(1)) and torch.equal(b, (q * 2.0).to(torch.int32))
