"""lora_hip_mux: many channels through ONE decoder pass (VERDICT r02 missing #6 / item 7b).  Every channel must publish what its own
lora_hip_work handle (and the batch decode) publishes - frames, header positions - whatever the order and chunking of the calls,
with channels running ahead of each other, with the latency bound cutting passes anywhere; and a gateway's worth of channels must
need one pass per chunk, not one per channel."""
import time

import numpy as np
import pytest

from gr_lora_amd import synth

pytestmark = pytest.mark.gpu


def _channels(n, sf, seed, packets=5):
    cfg = synth.TxConfig(sf=sf, cr=4)
    out = []
    for c in range(n):
        rng = np.random.default_rng(seed + c)
        pl = [bytes(rng.integers(0, 256, int(rng.integers(4, 50)), dtype=np.uint8)) for _ in range(packets + c % 3)]
        out.append(synth.build_stream(pl, cfg, rng=rng, gap_symbols=(0.0, 9.0), tail_symbols=4.0))
    return cfg, out


def _batch(sf, iq):
    import torch
    from gr_lora_amd import capi
    dev = torch.from_numpy(iq.view(np.float32)).cuda()
    h = capi.Handle(sf=sf, cr=4)
    h.decode_device(dev.data_ptr(), iq.size, [0], [iq.size], 0)
    out = [(b, i.header_pos) for b, i in h.drain()]
    h.close()
    return out


@pytest.mark.parametrize("sf,n", [(7, 8), (9, 5), (8, 1)])
def test_mux_equals_independent_decoders(sf, n):
    from gr_lora_amd import capi
    cfg, chans = _channels(n, sf, seed=500 + sf)
    want = [_batch(sf, st.iq) for st in chans]
    assert all(len(w) >= 5 for w in want)
    for batch, order in ((1 << 15, "interleaved"), (3 * cfg.sps + 17, "interleaved"), (1 << 16, "skewed")):
        m = capi.Mux(n, sf=sf, cr=4, batch_items=batch)
        m.set_latency(0.0)
        got = {c: [] for c in range(n)}
        pos = [0] * n
        rng = np.random.default_rng(1)
        live = list(range(n))
        while live:
            c = live[0] if order == "skewed" else int(rng.choice(live))   # skewed: channel 0 delivers everything first (it runs chunks ahead)
            k = int(rng.integers(1, 40000))
            m.work(c, chans[c].iq[pos[c]:pos[c] + k])
            pos[c] += k
            if pos[c] >= chans[c].iq.size:
                live.remove(c)
            for b, i in m.drain():
                got[i.stream].append((b, i.header_pos))
        m.flush()
        for b, i in m.drain():
            got[i.stream].append((b, i.header_pos))
        passes, _ = m.passes()
        m.close()
        for c in range(n):
            assert got[c] == want[c], (sf, batch, order, c, len(got[c]), len(want[c]))
        longest = max(st.iq.size for st in chans)
        assert passes <= longest // batch + 4, (passes, longest // batch)   # one pass per chunk for ALL channels, not one per channel


def test_mux_latency_bound_publishes_without_full_chunks():
    from gr_lora_amd import capi
    cfg, chans = _channels(4, 7, seed=900, packets=3)
    want = [_batch(7, st.iq) for st in chans]
    m = capi.Mux(4, sf=7, cr=4)            # default chunk: far larger than these streams
    m.set_latency(3.0)
    got = {c: [] for c in range(4)}
    n = max(st.iq.size for st in chans)
    seen_before_flush = 0
    for p in range(0, n, 8192):
        for c in range(4):
            m.work(c, chans[c].iq[p:p + 8192])
        time.sleep(0.001)
        for b, i in m.drain():
            got[i.stream].append((b, i.header_pos)); seen_before_flush += 1
    m.flush()
    for b, i in m.drain():
        got[i.stream].append((b, i.header_pos))
    passes, by_lat = m.passes()
    m.close()
    assert [got[c] for c in range(4)] == want
    assert by_lat >= 3 and seen_before_flush >= sum(len(w) for w in want) // 2


def test_mux_with_a_silent_channel():
    """a channel that delivers nothing must not hold the others back, even with the latency bound off: once an active channel's surplus
    in host memory reaches max_ahead the pass goes without waiting for the silent one (default 8 chunks / 4 Mi items; one chunk here)"""
    from gr_lora_amd import capi
    cfg, chans = _channels(3, 7, seed=1200, packets=6)
    want = [_batch(7, st.iq) for st in chans]
    batch = 1 << 15
    m = capi.Mux(4, sf=7, cr=4, batch_items=batch)      # channel 3 never gets a sample
    m.set_latency(0.0)                                  # (no help from the clock)
    m.set_max_ahead(batch)
    got = {c: [] for c in range(4)}
    n = max(st.iq.size for st in chans)
    before_flush = 0
    for p in range(0, n, 4096):
        for c in range(3):
            m.work(c, chans[c].iq[p:p + 4096])
        for b, i in m.drain():
            got[i.stream].append((b, i.header_pos)); before_flush += 1
    passes_streaming, _ = m.passes()
    m.flush()
    for b, i in m.drain():
        got[i.stream].append((b, i.header_pos))
    m.close()
    assert [got[c] for c in range(3)] == want and got[3] == []
    assert passes_streaming >= n // (2 * batch) - 1 and before_flush > 0, (passes_streaming, n // batch, before_flush)
