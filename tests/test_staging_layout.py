"""The byte layouts of ComposeSession's staging areas for the batched calls (compose_many,
compose_shared, screen) are pinned: every key and every offset, as recorded before the three
builders were folded onto one.  What is copied to and from the device is what these say.
The candidates' layout (candidates, screen_all) is pinned the same way, for its three-column
and its six-column selection, as recorded before the columns came from one table."""
import pytest

from semantic_merge_amd._lib import CAND_COLS, SCREEN_COLS, ComposeSession

BATCH = {  # ns
    (): {'n_total': 0, 'kind': 0, 'ts': 0, 'oid_hi': 0, 'oid_lo': 0, 'sym': 0, 'v0': 0, 'v1': 0, 'off': 0, 'n_a': 256, 'conf_off': 256, 'in_bytes': 512, 'q': 0, 'conf': 0, 'counts': 256, 'out_bytes': 256},
    (0,): {'n_total': 0, 'kind': 0, 'ts': 0, 'oid_hi': 0, 'oid_lo': 0, 'sym': 0, 'v0': 0, 'v1': 0, 'off': 0, 'n_a': 256, 'conf_off': 512, 'in_bytes': 768, 'q': 0, 'conf': 0, 'counts': 256, 'out_bytes': 272},
    (1,): {'n_total': 1, 'kind': 0, 'ts': 256, 'oid_hi': 512, 'oid_lo': 768, 'sym': 1024, 'v0': 1280, 'v1': 1536, 'off': 1792, 'n_a': 2048, 'conf_off': 2304, 'in_bytes': 2560, 'q': 256, 'conf': 1024, 'counts': 1280, 'out_bytes': 1296},
    (2048, 1, 255, 0): {'n_total': 2304, 'kind': 0, 'ts': 2304, 'oid_hi': 20736, 'oid_lo': 39168, 'sym': 57600, 'v0': 66816, 'v1': 76032, 'off': 85248, 'n_a': 85504, 'conf_off': 85760, 'in_bytes': 86016, 'q': 9216, 'conf': 36864, 'counts': 46336, 'out_bytes': 46400},
}
SHARED = {  # (n_total, n_shared, m)
    (0, 0, 0): {'n_total': 0, 'kind': 0, 'ts': 0, 'oid_hi': 0, 'oid_lo': 0, 'sym': 0, 'v0': 0, 'v1': 0, 'off': 0, 'conf_off': 256, 'in_bytes': 512, 'q': 0, 'conf': 0, 'counts': 256, 'out_bytes': 256},
    (5, 5, 1): {'n_total': 5, 'kind': 0, 'ts': 256, 'oid_hi': 512, 'oid_lo': 768, 'sym': 1024, 'v0': 1280, 'v1': 1536, 'off': 1792, 'conf_off': 2048, 'in_bytes': 2304, 'q': 256, 'conf': 1024, 'counts': 1280, 'out_bytes': 1296},
    (2049, 1, 3): {'n_total': 2049, 'kind': 0, 'ts': 2304, 'oid_hi': 18944, 'oid_lo': 35584, 'sym': 52224, 'v0': 60672, 'v1': 69120, 'off': 77568, 'conf_off': 77824, 'in_bytes': 78080, 'q': 8448, 'conf': 33792, 'counts': 50432, 'out_bytes': 50480},
}
SCREEN = {  # (n_total, n_logs, n_pairs, n_conf)
    (0, 0, 0, 0): {'n_total': 0, 'kind': 0, 'ts': 0, 'oid_hi': 0, 'oid_lo': 0, 'sym': 0, 'v0': 0, 'col_bytes': 0, 'log_off': 0, 'pair_a': 256, 'pair_b': 256, 'conf_off': 256, 'in_bytes': 512, 'conf': 0, 'counts': 256, 'out_bytes': 256},
    (7, 2, 1, 0): {'n_total': 7, 'kind': 0, 'ts': 256, 'oid_hi': 512, 'oid_lo': 768, 'sym': 1024, 'v0': 1280, 'col_bytes': 1536, 'log_off': 1536, 'pair_a': 1792, 'pair_b': 2048, 'conf_off': 2304, 'in_bytes': 2560, 'conf': 0, 'counts': 256, 'out_bytes': 264},
    (4096, 3, 3, 5): {'n_total': 4096, 'kind': 0, 'ts': 4096, 'oid_hi': 36864, 'oid_lo': 69632, 'sym': 102400, 'v0': 118784, 'col_bytes': 135168, 'log_off': 135168, 'pair_a': 135424, 'pair_b': 135680, 'conf_off': 135936, 'in_bytes': 136192, 'conf': 0, 'counts': 256, 'out_bytes': 280},
}
_CAND_OUT = {  # (n_logs, cap): the output side, the same for either selection
    (1, 1): {'conf': 0, 'counts': 0, 'out_bytes': 1024, 'log_info': 256, 'pair_a': 512, 'pair_b': 768},
    (2, 1): {'conf': 0, 'counts': 0, 'out_bytes': 1024, 'log_info': 256, 'pair_a': 512, 'pair_b': 768},
    (41, 1024): {'conf': 0, 'counts': 0, 'out_bytes': 8704, 'log_info': 256, 'pair_a': 512, 'pair_b': 4608},
}
CAND3 = {  # (n_total, n_logs, cap): kind, sym, v0
    (0, 1, 1): {'n_total': 0, 'kind': 0, 'sym': 0, 'v0': 0, 'log_off': 0, 'in_bytes': 256, **_CAND_OUT[1, 1]},
    (7, 2, 1): {'n_total': 7, 'kind': 0, 'sym': 256, 'v0': 512, 'log_off': 768, 'in_bytes': 1024, **_CAND_OUT[2, 1]},
    (4096, 41, 1024): {'n_total': 4096, 'kind': 0, 'sym': 4096, 'v0': 20480, 'log_off': 36864, 'in_bytes': 37376, **_CAND_OUT[41, 1024]},
}
CAND6 = {  # (n_total, n_logs, cap): the screen's six columns
    (0, 1, 1): {'n_total': 0, 'kind': 0, 'ts': 0, 'oid_hi': 0, 'oid_lo': 0, 'sym': 0, 'v0': 0, 'log_off': 0, 'in_bytes': 256, **_CAND_OUT[1, 1]},
    (7, 2, 1): {'n_total': 7, 'kind': 0, 'ts': 256, 'oid_hi': 512, 'oid_lo': 768, 'sym': 1024, 'v0': 1280, 'log_off': 1536, 'in_bytes': 1792, **_CAND_OUT[2, 1]},
    (4096, 41, 1024): {'n_total': 4096, 'kind': 0, 'ts': 4096, 'oid_hi': 36864, 'oid_lo': 69632, 'sym': 102400, 'v0': 118784, 'log_off': 135168, 'in_bytes': 135680, **_CAND_OUT[41, 1024]},
}


@pytest.mark.parametrize("ns", list(BATCH))
def test_batch_layout(ns):
    assert ComposeSession._batch_layout(list(ns)) == BATCH[ns]


@pytest.mark.parametrize("shape", list(SHARED))
def test_shared_layout(shape):
    assert ComposeSession._shared_layout(*shape) == SHARED[shape]


@pytest.mark.parametrize("shape", list(SCREEN))
def test_screen_layout(shape):
    assert ComposeSession._screen_layout(*shape) == SCREEN[shape]


@pytest.mark.parametrize("shape", list(CAND3))
def test_cand_layout_three_columns(shape):
    assert [c[0] for c in CAND_COLS] == ["kind", "sym", "v0"]
    assert ComposeSession._cand_layout(*shape, CAND_COLS) == CAND3[shape]


@pytest.mark.parametrize("shape", list(CAND6))
def test_cand_layout_six_columns(shape):
    assert [c[0] for c in SCREEN_COLS] == ["kind", "ts", "oid_hi", "oid_lo", "sym", "v0"]
    assert ComposeSession._cand_layout(*shape, SCREEN_COLS) == CAND6[shape]
    # the six columns lie where the screen has them: screen_all's second call reads them there
    screen = ComposeSession._screen_layout(shape[0], shape[1], 1)
    assert all(CAND6[shape][c[0]] == screen[c[0]] for c in SCREEN_COLS)
    assert CAND6[shape]["log_off"] == screen["log_off"]
