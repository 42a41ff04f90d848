"""GPU: grp_bgzf_inflate (csrc/grp_inflate.inc) — raw DEFLATE payloads inflated one wave per block, CRC32 on the device.
The expectation is Python's zlib everywhere (tests/bgzf_cases.py): every good payload is inflated by zlib first and that
text is what the device must return; every bad one is refused by zlib too."""
import numpy as np
import pytest

import bgzf_cases as B
from helpers import default_seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds())
    yield e
    e.close()


@pytest.fixture(scope="module")
def good():
    """name -> (payload, text, crc32): every text in every compressor form, and the hand-written blocks"""
    out = {}
    for tn, t in B.texts().items():
        for fn, kw in B.FORMS.items():
            out[tn + "/" + fn] = B.deflate(t, **kw)
        out[tn + "/flushed"] = B.flushed(t)
    out.update(("hand/" + n, p) for n, p in B.hand_written().items())
    res, texts = {}, B.texts()
    for name, p in out.items():
        text, crc = B.confirm_good(p)  # zlib's word, not the input's
        assert name.startswith("hand/") or text == texts[name.split("/")[0]]
        res[name] = (p, text, crc)
    return res


def _pack(items, gap=0):
    """payloads one after the other (with `gap` + i % 4 bytes of other data between them: every alignment) -> (comp, blocks)"""
    comp, blocks = bytearray(), []
    for i, (p, text_len, crc) in enumerate(items):
        comp += b"\xa5" * ((gap + i) % 4 if gap else 0)
        blocks.append((len(comp), len(p), text_len, crc))
        comp += p
    return bytes(comp), blocks


@pytest.mark.parametrize("form", list(B.FORMS) + ["flushed", "hand"])
def test_inflate_matches_zlib(eng, good, form):
    names = [n for n in good if n.endswith("/" + form) or n.startswith(form + "/")]
    assert len(names) >= 5
    comp, blocks = _pack([(good[n][0], len(good[n][1]), good[n][2]) for n in names], gap=1)
    text = eng.bgzf_inflate(comp, blocks)
    at = 0
    for n in names:
        exp = good[n][1]
        assert text[at:at + len(exp)] == exp, n
        at += len(exp)
    assert at == len(text)


def test_single_blocks_of_the_edge_lengths(eng, good):
    for n in (0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65535, 65536):
        p, text, crc = good["len%d/level6" % n]
        assert len(text) == n
        assert eng.bgzf_inflate(p, [(0, len(p), n, crc)]) == text


def test_one_call_with_300_mixed_blocks(eng, good):
    rng = np.random.default_rng(5)
    fq = B.texts()["fastq"]
    items = [(p, len(t), c) for p, t, c in good.values()]
    expect = [t for _, t, _ in good.values()]
    while len(items) < 300:  # odd lengths: the texts start at every byte alignment
        a, n = int(rng.integers(0, 30000)), int(rng.integers(1, 30000)) | 1
        p = B.deflate(fq[a:a + n], int(rng.choice([1, 6, 9])))
        t, c = B.confirm_good(p)
        items.append((p, len(t), c))
        expect.append(t)
    order = rng.permutation(len(items))
    items, expect = [items[i] for i in order], [expect[i] for i in order]
    comp, blocks = _pack(items, gap=3)
    before = eng.bgzf_stats()
    text = eng.bgzf_inflate(comp, blocks)
    assert text == b"".join(expect)
    assert len({sum(len(t) for t in expect[:i]) % 4 for i in range(len(expect))}) == 4
    after = eng.bgzf_stats()
    assert after["blocks"] - before["blocks"] == len(items)
    assert after["comp_bytes"] - before["comp_bytes"] == len(comp)
    assert after["text_bytes"] - before["text_bytes"] == len(text)
    assert after["kernel_us"] > before["kernel_us"]


@pytest.mark.parametrize("name", ["wrong_crc", "text_len_plus_1", "text_len_minus_1", "cut_by_5", "block_type_3", "stored_len_mismatch",
                                  "oversubscribed_code_lengths", "incomplete_literal_set", "match_at_position_0", "distance_symbol_30"])
def test_refused_inputs_name_the_block(eng, native, good, name):
    bad = B.refused()[name]  # (zlib has turned it down: bgzf_cases.refused)
    ok = [(p, len(t), c) for p, t, c in (good["fastq/level6"], good["bytes/level1"], good["len257/fixed"])]
    comp, blocks = _pack([ok[0], ok[1], bad, ok[2]], gap=2)
    with pytest.raises(native.GrpError) as e:
        eng.bgzf_inflate(comp, blocks)
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_block == 2, str(e.value)
    assert "block 2" in str(e.value)
    # the engine goes on: the good blocks alone
    comp, blocks = _pack(ok, gap=2)
    assert eng.bgzf_inflate(comp, blocks) == b"".join(t for t in (good["fastq/level6"][1], good["bytes/level1"][1], good["len257/fixed"][1]))


def test_argument_errors_launch_nothing(eng, native, good):
    p, text, crc = good["fastq/level6"]
    before = eng.bgzf_stats()
    for blocks, cap in (([(0, len(p), len(text), crc), (5, len(p) - 4, len(text), crc)], None),  # comp_off + comp_len > n_comp
                        ([(0, len(p), 65537, crc)], None),                                      # text_len > 65536
                        ([(0, len(p), len(text), crc)] * 2, 2 * len(text) - 1)):                # sum of the texts > text_cap
        with pytest.raises(native.GrpError) as e:
            eng.bgzf_inflate(p, blocks, text_cap=cap)
        assert e.value.code == native.GRP_ERR_INVALID
    assert eng.bgzf_stats() == before
    assert eng.bgzf_inflate(p, [(0, len(p), len(text), crc)]) == text
