"""The encoder's dictionary re-base (lzo1x_enc_rebase.h: when, and to where;
rebase_dict in lzo1x_encode_fast.hip: the pipelined rewrite and the bitmap
refresh) through the three throughput encoder kernels, byte for byte against
the oracle: the block sizes around the first re-base, blocks that re-base
several times with entries living across a re-base at distances 0xBFFE ..
0xC001, and stale entries behind a refreshed bitmap.

test_enc_rebase.rebase_blocks() builds the inputs and tests/test_enc_rebase.py
checks on the CPU that each hits its edge."""
from __future__ import annotations

import pytest

from pomegranate_amd import lzo
from test_enc_rebase import rebase_blocks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def cases(oracle):
    named = rebase_blocks()
    return [n for n, _, _ in named], [b for _, b, _ in named], [oracle.compress(b) for _, b, _ in named]


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


@pytest.mark.parametrize("kernel", ["gdict_one_wave", "gdict_two_wave", "lds"])
def test_rebase_vs_oracle(dev, cases, debug_env, kernel):
    import gpu_util as gu
    names, blocks, want = cases
    debug_env("enc_waves=2" if kernel == "gdict_two_wave" else "enc_waves=1")
    src = gu.device_batch(torch, blocks, dev)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=0xA5)
    olen = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    st = torch.full((len(blocks),), 99, dtype=torch.int32, device=dev)
    scr = None
    if kernel != "lds":                                  # (a dirty scratch: dictionaries of garbage)
        scr = torch.full((lzo.compress_scratch_bytes(len(blocks)),), 0x5A, dtype=torch.uint8, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [0] * len(blocks)
    comps = gu.fetch(dst, olen)
    bad = [n for n, c, w in zip(names, comps, want) if c != w]
    assert not bad, f"{len(bad)} of {len(blocks)} differ from the oracle, first {bad[:8]}"
