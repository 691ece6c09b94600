"""GPU: seg_ema_update / seg_ema_swap (csrc/adam.hip) through seg_amd.EMA and through call(...) directly.

Tensors: sizes 1, 3, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 3 and (96, 16, 1, 1) -- the block (256) and chunk
(4096) edges -- plus one int64 buffer that must be ignored.  Every fp32 tensor is a contiguous slice of one flat
buffer with 64-element sentinel gaps, for the sources and for the shadows; the gaps must be unchanged after every
launch.

Bound against float64: the reference recurrence is e64 += double(w_fp32) * (p - e64); after k updates, elementwise
|e - e64| <= k * 2^-21 * M, M the largest |e| or |p| the element has seen.  Per update: one rounding of p - e
(<= 2^-24 * 2M), at most one of the product and one of the sum, <= 5 * 2^-24 * M for w <= 1; the map contracts, so
the errors at most add.  (A CPU fp32 run of 20 updates stays at a quarter of the tighter k * 2^-22 over
w in {1e-4, 1e-3, 0.1, 0.5}.)  k = 5, decay in {0.9999, 0.9, 0.1}.
"""
import pytest
import torch
from torch import nn

from seg_amd import EMA
from seg_amd._lib import lib
from seg_amd.optim import _CHUNK, _chunk_map

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1,), (3,), (255,), (256,), (257,), (4095,), (4096,), (4097,), (2 * 4096 + 3,), (96, 16, 1, 1)]
GAP = 64
SENTINEL = -12345.5


def _flat_views(fill_seed):
    """(flat buffer, views): every shape a contiguous slice of `flat`, a GAP of sentinels before, between and after."""
    total = GAP + sum(torch.Size(s).numel() + GAP for s in SHAPES)
    flat = torch.full((total,), SENTINEL, dtype=torch.float32)
    g = torch.Generator().manual_seed(fill_seed)
    views, mask, off = [], torch.ones(total, dtype=torch.bool), GAP
    for s in SHAPES:
        n = torch.Size(s).numel()
        flat[off:off + n] = torch.randn(n, generator=g) * 3
        mask[off:off + n] = False
        off += n + GAP
    flat = flat.to(DEV)
    off = GAP
    for s in SHAPES:
        n = torch.Size(s).numel()
        views.append(flat[off:off + n].view(s))
        off += n + GAP
    return flat, views, mask.to(DEV)


class Bag(nn.Module):
    """Parameters and buffers that are views of one flat buffer, and an int64 buffer."""

    def __init__(self, views):
        super().__init__()
        for i, v in enumerate(views):
            if i % 3 == 2:
                self.register_buffer(f"b{i}", v)
            else:
                self.register_parameter(f"p{i}", nn.Parameter(v))  # shares the view's storage
        self.register_buffer("count", torch.arange(7, dtype=torch.int64, device=DEV))


def _setup(decay, seed=1, same=False):
    """(bag, ema, source flat, shadow flat, gap mask): the shadows re-homed into a sentinel-gapped buffer too."""
    pflat, pviews, mask = _flat_views(seed)
    bag = Bag(pviews)
    ema = EMA(bag, decay=decay)
    eflat, eviews, _ = _flat_views(seed if same else seed + 100)
    assert len(ema.shadows) == len(SHAPES) and ema.names == [k for k in bag.state_dict() if k != "count"]
    order = {k: i for i, k in enumerate(f"b{i}" if i % 3 == 2 else f"p{i}" for i in range(len(SHAPES)))}
    ema.shadows = [eviews[order[k]] for k in ema.names]
    ema._key = None  # the table is rebuilt over the re-homed shadows at the next launch
    return bag, ema, pflat, eflat, mask


def _gaps_intact(*flats_and_mask):
    *flats, mask = flats_and_mask
    return all(bool((f[mask] == SENTINEL).all()) for f in flats)


def _table(pairs):
    rows = [(e.data_ptr(), p.data_ptr(), p.numel()) for e, p in pairs]
    return (torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(DEV),
            _chunk_map([p.numel() for _, p in pairs], DEV))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("decay", [0.9999, 0.9, 0.1])
def test_five_updates_against_float64(decay):
    bag, ema, pflat, eflat, mask = _setup(decay)
    w = float(torch.tensor(1.0 - decay, dtype=torch.float32))
    srcs = dict(bag.state_dict())
    e64 = {k: e.double().clone() for k, e in zip(ema.names, ema.shadows)}
    M = {k: torch.maximum(e64[k].abs(), srcs[k].double().abs()) for k in ema.names}
    g = torch.Generator().manual_seed(77)
    K = 5
    for step in range(K):
        for k in ema.names:  # the sources move between updates, as under training
            srcs[k].add_((0.5 * torch.randn(srcs[k].shape, generator=g)).to(DEV))
        before = {k: srcs[k].clone() for k in ema.names}
        ema.update()
        torch.cuda.synchronize()
        for k in ema.names:
            assert torch.equal(srcs[k], before[k]), k  # p is never written by the update
            e64[k] += w * (srcs[k].double() - e64[k])
            M[k] = torch.maximum(M[k], torch.maximum(srcs[k].double().abs(), e64[k].abs()))
        assert _gaps_intact(pflat, eflat, mask)
    assert ema.num_updates == K
    worst = 0.0
    for k, e in zip(ema.names, ema.shadows):
        err = (e.double() - e64[k]).abs()
        bound = K * 2.0 ** -21 * M[k]
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (k, float(err.max()))
    print(f"decay {decay}: worst error / bound after {K} updates {worst:.3f}")
    assert torch.equal(bag.count, torch.arange(7, dtype=torch.int64, device=DEV))


def test_decay_one_leaves_the_shadows_unchanged():
    bag, ema, pflat, eflat, mask = _setup(1.0)
    want = eflat.clone()
    ema.update()
    torch.cuda.synchronize()
    assert torch.equal(eflat, want)


def test_shadows_equal_to_their_sources_stay_equal():
    bag, ema, pflat, eflat, mask = _setup(0.9, same=True)
    assert torch.equal(eflat, pflat)
    for _ in range(3):
        ema.update()
    torch.cuda.synchronize()
    assert torch.equal(eflat, pflat)


def test_two_runs_from_the_same_state_agree():
    out = []
    for _ in range(2):
        bag, ema, pflat, eflat, mask = _setup(0.9, seed=4)
        for _ in range(3):
            ema.update()
        torch.cuda.synchronize()
        out.append(eflat.clone())
    assert torch.equal(out[0], out[1])


def test_swap_exchanges_and_a_second_swap_restores():
    bag, ema, pflat, eflat, mask = _setup(0.9)
    p_old, e_old = pflat.clone(), eflat.clone()
    ema.swap()
    torch.cuda.synchronize()
    assert _gaps_intact(pflat, eflat, mask)
    assert torch.equal(eflat[~mask], p_old[~mask]) and torch.equal(pflat[~mask], e_old[~mask])
    by_name = dict(bag.state_dict())
    for k, e in zip(ema.names, ema.shadows):  # and as the model sees it: no tensor was rebound
        assert pflat.data_ptr() <= by_name[k].data_ptr() < pflat.data_ptr() + 4 * pflat.numel(), k
        assert eflat.data_ptr() <= e.data_ptr() < eflat.data_ptr() + 4 * eflat.numel(), k
    ema.swap()
    torch.cuda.synchronize()
    assert torch.equal(pflat, p_old) and torch.equal(eflat, e_old)
    with ema.applied():
        torch.cuda.synchronize()
        assert torch.equal(eflat[~mask], p_old[~mask]) and torch.equal(pflat[~mask], e_old[~mask])
    torch.cuda.synchronize()
    assert torch.equal(pflat, p_old) and torch.equal(eflat, e_old)
    assert torch.equal(bag.count, torch.arange(7, dtype=torch.int64, device=DEV))


def test_skip_flag():
    bag, ema, pflat, eflat, mask = _setup(0.9)
    p_old, e_old = pflat.clone(), eflat.clone()
    ema.update(skip_if_nonzero=torch.tensor([2.0], device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(pflat, p_old) and torch.equal(eflat, e_old)  # nothing touched
    assert ema.num_updates == 1
    ema.undo_update_count()
    assert ema.num_updates == 0
    ema.update(skip_if_nonzero=torch.zeros(1, device=DEV))  # a flag holding 0 behaves as no flag
    torch.cuda.synchronize()
    with_zero = eflat.clone()
    bag2, ema2, pflat2, eflat2, _ = _setup(0.9)
    ema2.update()
    torch.cuda.synchronize()
    assert torch.equal(with_zero, eflat2) and not torch.equal(with_zero, e_old)
    assert torch.equal(pflat, p_old)
    with pytest.raises(ValueError):
        ema.update(skip_if_nonzero=torch.zeros(1))  # a host tensor cannot be read by the kernel


def test_direct_calls_edge_cases():
    pflat, pviews, mask = _flat_views(1)
    eflat, eviews, _ = _flat_views(2)
    table, chunks = _table(list(zip(eviews, pviews)))
    p_old, e_old = pflat.clone(), eflat.clone()
    h = lib()
    n = chunks.shape[0]
    assert n == sum(-(-torch.Size(s).numel() // _CHUNK) for s in SHAPES)
    # nchunks == 0: success, no launch; chunk == 0 and nchunks < 0: an error, nothing written
    assert h.seg_ema_update(table.data_ptr(), chunks.data_ptr(), 0, _CHUNK, 0.5, None, _stream()) == 0
    assert h.seg_ema_swap(table.data_ptr(), chunks.data_ptr(), 0, _CHUNK, _stream()) == 0
    assert h.seg_ema_update(table.data_ptr(), chunks.data_ptr(), n, 0, 0.5, None, _stream()) == 1
    assert h.seg_ema_swap(table.data_ptr(), chunks.data_ptr(), n, 0, _stream()) == 1
    assert h.seg_ema_update(table.data_ptr(), chunks.data_ptr(), -1, _CHUNK, 0.5, None, _stream()) == 1
    assert h.seg_ema_swap(table.data_ptr(), chunks.data_ptr(), -1, _CHUNK, _stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(pflat, p_old) and torch.equal(eflat, e_old)
    # one direct update (w = 0.25, exact in fp32) within the one-update bound, then one direct swap
    assert h.seg_ema_update(table.data_ptr(), chunks.data_ptr(), n, _CHUNK, 0.25, None, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pflat, p_old) and _gaps_intact(pflat, eflat, mask)
    e64 = e_old.double() + 0.25 * (p_old.double() - e_old.double())
    M = torch.maximum(torch.maximum(e_old.double().abs(), p_old.double().abs()), e64.abs())
    err = (eflat.double() - e64).abs()[~mask]
    assert bool((err <= 2.0 ** -21 * M[~mask]).all())
    e_new = eflat.clone()
    assert h.seg_ema_swap(table.data_ptr(), chunks.data_ptr(), n, _CHUNK, _stream()) == 0
    torch.cuda.synchronize()
    assert _gaps_intact(pflat, eflat, mask)
    assert torch.equal(eflat[~mask], p_old[~mask]) and torch.equal(pflat[~mask], e_new[~mask])


def test_refusals():
    base = nn.Conv2d(4, 6, 3).to(DEV)
    EMA(base)  # contiguous fp32: fine
    half = nn.Conv2d(4, 6, 3).to(DEV).half()
    with pytest.raises(NotImplementedError):
        EMA(half)
    strided = nn.Conv2d(4, 6, 3).to(DEV)
    strided.weight.data = torch.randn(6, 3, 3, 4, device=DEV).permute(0, 3, 1, 2)
    assert not strided.weight.is_contiguous()
    with pytest.raises(NotImplementedError):
        EMA(strided)
    ema = EMA(base)
    base.weight.data = torch.randn(6, 3, 3, 4, device=DEV).permute(0, 3, 1, 2)  # rebound to something refused
    before = [e.clone() for e in ema.shadows]
    with pytest.raises(NotImplementedError):
        ema.update()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ema.shadows, before))
