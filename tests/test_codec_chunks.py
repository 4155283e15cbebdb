"""CPU: the two host rules every codec wrapper of ops shares -- the greedy grouping of consecutive items under a scratch budget
(ops._budget_chunks) and what counts as a file or a list of files (ops._byte_files)."""
import pytest

from cartoonsegmentation_amd import ops


@pytest.mark.parametrize("own, budget, groups", [
    ([5, 5, 5, 20, 1], 10, [(0, 2), (2, 1), (3, 1), (4, 1)]),      # an item above the budget is still taken, alone
    ([], 10, []),
    ([7], 1, [(0, 1)]),
    ([4, 4, 4], 8, [(0, 2), (2, 1)]),                              # a group may reach the budget exactly
])
def test_budget_chunks(own, budget, groups):
    assert list(ops._budget_chunks(own, budget)) == groups


def test_budget_chunks_cover_every_item_once_in_order():
    own = [3, 9, 1, 1, 1, 12, 2, 8, 8, 0, 5]
    for budget in (0, 1, 8, 10, 16, 100):
        got = list(ops._budget_chunks(own, budget))
        assert [i for i, _ in got] == [sum(k for _, k in got[:j]) for j in range(len(got))]
        assert sum(k for _, k in got) == len(own) and all(k >= 1 for _, k in got)
        for i, k in got:
            assert k == 1 or sum(own[i:i + k]) <= budget
            assert i + k == len(own) or sum(own[i:i + k + 1]) > budget            # the group could not take one more


def test_byte_files():
    data = b"\x89PNG"
    for one in (data, bytearray(data), memoryview(data)):
        single, datas = ops._byte_files(one, "png_decode")
        assert single and len(datas) == 1 and datas[0] is one
    single, datas = ops._byte_files([data, bytearray(data)], "png_decode")
    assert not single and len(datas) == 2 and datas[0] is data
    assert ops._byte_files([], "png_decode") == (False, [])
    single, datas = ops._byte_files((d for d in [data]), "png_decode")      # any iterable of files is a list of files
    assert not single and datas == [data]
    with pytest.raises(TypeError, match=r"^webp_decode: bytes or a list of bytes expected \(got int\)$"):
        ops._byte_files([data, 5], "webp_decode")
    with pytest.raises(TypeError, match=r"^jpeg_decode: bytes or a list of bytes expected \(got str\)$"):
        ops._byte_files(["a file name"], "jpeg_decode")
