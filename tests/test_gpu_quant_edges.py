"""k_loop's quantise+count pass on the DEVICE (mp3mi_debug_quantize_count, csrc/k_loop_qc.hip) against the oracle on every granule
of the edge sets S1..S7 (tests/quant_edges.py) at every rate: ix, the rescaled xr and every field, bit for bit.  And the sets
reach what they are for: the rare tier on the boundary sets, the all-zero shortcut, the clamp at the table's end, every Huffman
group and linbits table a maximum of at most 2047 can select."""
import numpy as np
import pytest

import quant_edges as qe
from mp3common import Oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate", qe.RATES)
def test_device_pass_is_the_oracle_at_the_edges(product, rate):
    S = qe.Sets(rate)
    ix, xo, f = qe.run_oracle(Oracle().lib, rate, S.xr, S.gran)
    idx = np.arange(len(S.xr))
    rc, hix, hxo, hf = qe.run_hook(product.lib, rate, S.xr, S.gran)
    assert rc == 0
    msg = qe.first_mismatch(S, idx, hix, hxo, hf, ix, xo, f)
    assert msg is None, msg
    F = qe.QCI
    # coverage: the boundary sets exercise the rare tier, the lines on a boundary among those it settles
    for name in ("S1", "S2"):
        w = S.set == name
        assert hf[w, F["rare_tier"]].mean() > 0.9, (name, hf[w, F["rare_tier"]].mean())
        assert hf[w, F["n_differ"]].sum() > 0.5 * 576 * w.sum() * (0.4 if name == "S1" else 0.1), name
    assert hf[:, F["all_zero"]].any() and hf[:, F["over"]].any()
    # the all-zero shortcut at its threshold: taken and not taken among the S3 granules that quantise to nothing
    s3z = (S.set == "S3") & (np.abs(ix).max(axis=1) == 0)
    assert hf[s3z, F["all_zero"]].any() and not hf[s3z, F["all_zero"]].all()
    # every descriptor class (Huffman group and linbits pair) of long-block regions and of both short-block regions
    s456 = np.isin(S.set, ["S4", "S5", "S6"])
    longb = s456 & (S.gran[:, 1] != 2)
    cls_long = set(qe.desc_class(qe.region_maxima(ix[longb], f[longb])).ravel().tolist())
    shortb = s456 & (S.gran[:, 1] == 2)
    cls_short = set(qe.desc_class(hf[shortb][:, [F["m1"], F["m2"]]]).ravel().tolist())
    assert cls_long >= set(range(27)) and cls_short >= set(range(27)), (sorted(set(range(27)) - cls_long), sorted(set(range(27)) - cls_short))
    tables = set(hf[s456][:, [F["table_select0"], F["table_select1"], F["table_select2"]]].ravel().tolist())
    assert tables >= set(range(16, 31)) | {1, 2, 3, 5, 6, 7, 10, 13, 15}, sorted(tables)
