"""CPU suite: the form in which RANSAC's batch loop uploads its index triples (csrc/tdv_internal.hpp: triple_pack; csrc/ctx.hip:
TripleStream::next_batch_packed, exported as tdv_sample_triples_batch).  Clouds of at most 2^21 points send one 64-bit word per
triple - three 21-bit indices and the valid bit - instead of an int4; the words unpack to the index stream of tdv_sample_triples,
the valid bit is "three distinct indices" (registration.cpp:240), and a cloud one point larger keeps the int4 form."""
import numpy as np
import pytest

PACK_MAX = 2 ** 21


@pytest.mark.parametrize("n", [3, 640, 200000, PACK_MAX - 1, PACK_MAX])
def test_packed_triples_unpack_to_the_index_stream(tdv, n):
    count = 5000
    raw, packed = tdv.sample_triples_batch(n, count)
    assert packed and raw.dtype == np.uint64 and raw.shape == (count,)
    tri, valid = tdv.unpack_triples(raw, packed)
    ref = tdv.sample_triples(n, count)
    assert np.array_equal(tri, ref), n
    distinct = (ref[:, 0] != ref[:, 1]) & (ref[:, 1] != ref[:, 2]) & (ref[:, 0] != ref[:, 2])
    assert np.array_equal(valid, distinct), n
    assert not ((raw >> np.uint64(63)) != 0)[~distinct].any()
    if n == 3:
        assert (~distinct).sum() > count // 2          # 7 of 9 triples over three points repeat an index
    if n >= PACK_MAX - 1:
        assert int(tri.max()) >= 2 ** 20               # the top index bit is in use


def test_packed_triples_other_seeds_and_chunks(tdv):
    for seed, n, count in ((7, 1000, 1), (7, 1000, 1025), (123, 32129, 70000)):
        raw, packed = tdv.sample_triples_batch(n, count, seed=seed)
        tri, _ = tdv.unpack_triples(raw, packed)
        assert packed and np.array_equal(tri, tdv.sample_triples(n, count, seed=seed)), (seed, n, count)


def test_a_cloud_past_the_packing_limit_keeps_int4(tdv):
    n, count = PACK_MAX + 1, 3000
    raw, packed = tdv.sample_triples_batch(n, count)
    assert not packed and raw.dtype == np.int32 and raw.shape == (count, 4)
    tri, valid = tdv.unpack_triples(raw, packed)
    ref = tdv.sample_triples(n, count)
    assert np.array_equal(tri, ref)
    assert np.array_equal(valid, (ref[:, 0] != ref[:, 1]) & (ref[:, 1] != ref[:, 2]) & (ref[:, 0] != ref[:, 2]))
    assert int(tri.max()) <= PACK_MAX                  # (an index of 2^21 itself would not fit 21 bits)


def test_sample_triples_batch_rejects_bad_arguments(tdv):
    with pytest.raises(tdv.TdvError):
        tdv.sample_triples_batch(0, 4)
    with pytest.raises(tdv.TdvError):
        tdv.sample_triples_batch(2 ** 31 + 1, 4)
