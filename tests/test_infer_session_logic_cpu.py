"""Host logic of the inference session (inference.py): token and frame buckets, graph keys, eviction and counters."""
import pytest


def test_padded_tokens(pkg):
    f = pkg.inference.padded_tokens
    assert [f(n, [32, 64, 128]) for n in (1, 32, 33, 64, 100, 128)] == [32, 32, 64, 64, 128, 128]
    assert f(129, [32, 64, 128]) == 256 and f(300, [32, 64, 128]) == 384         # multiples of the largest step beyond it


def test_frame_capacity(pkg):
    f = pkg.inference.frame_capacity
    assert f(1, 64) == (64, 64) and f(64, 64) == (64, 64) and f(65, 64) == (128, 128)
    assert f(100, 1) == (100, 100)
    assert f(100, 64, max_len=1000) == (128, 128)
    assert f(100, 64, max_len=110) == (110, 110)       # capped by max_len
    assert f(100, 64, max_len=50) == (100, 50)         # the flow still sees every predicted frame; the decoder max_len


def test_cache_warmup_capture_replay(pkg):
    c = pkg.inference.GraphCache(8)
    p = ("P", 1, 32, False, True)
    s = ("S", p, 64, 64)
    assert c.lookup(p)[1] == "eager" and c.lookup(s, parent=p)[1] == "eager"
    ent, act = c.lookup(p)
    assert act == "capture"
    c.captured(ent, object())
    ent, act = c.lookup(s, parent=p)
    assert act == "capture"
    c.captured(ent, object())
    assert c.lookup(p)[1] == "replay" and c.lookup(s, parent=p)[1] == "replay"
    assert c.stats == dict(calls=0, graphs=2, hits=2, captures=2, warmups=2, evictions=0, fallbacks=0)


def _capture(c, key, parent=None):
    c.lookup(key, parent)
    ent, act = c.lookup(key, parent)
    assert act == "capture"
    c.captured(ent, object())


def test_cache_eviction_lru_and_children(pkg):
    c = pkg.inference.GraphCache(3)
    pa, pb = ("P", 1, 32, False, True), ("P", 1, 64, False, True)
    sa1, sa2, sa3 = ("S", pa, 64, 64), ("S", pa, 128, 128), ("S", pa, 192, 192)
    sb1, sb2 = ("S", pb, 64, 64), ("S", pb, 128, 128)
    _capture(c, pa)
    _capture(c, sa1, pa)
    _capture(c, sa2, pa)
    assert c.stats["graphs"] == 3
    c.lookup(sa2, pa)                                  # sa2 and its parent are recent: the least recently used graph is sa1
    _capture(c, pb)
    assert sa1 not in c.entries and c.stats["graphs"] == 3 and c.stats["evictions"] == 1
    assert c.lookup(sa3, pa)[1] == "eager"             # seen once, no graph yet
    _capture(c, sb1, pb)                               # LRU graph: sa2
    assert sa2 not in c.entries
    _capture(c, sb2, pb)                               # LRU graph: pa, and every S key under it goes with it
    assert pa not in c.entries and sa3 not in c.entries
    assert set(c.entries) == {pb, sb1, sb2} and c.stats["graphs"] == 3 and c.stats["evictions"] == 3


def test_cache_rejects_tiny_limit(pkg):
    with pytest.raises(ValueError):
        pkg.inference.GraphCache(1)


def test_session_refuses_train_mode(pkg):
    import torch

    class Net(torch.nn.Module):
        upsample_rates = [4]

    net = Net()
    net.lin = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match="eval mode"):
        pkg.inference.Synthesizer(net.train())


def test_fallback_decision(pkg):
    """Calls predicted longer than max_frames go to eager infer(); the session only decides from the host lengths."""
    f = pkg.inference.Synthesizer.needs_fallback
    assert not f(4096, 4096) and f(4097, 4096)
