"""A span's reading does not depend on where the span stands in the caller's list (peaq_batch_run_windows,
peaq_batch_run_adv_spans; gstpeaq_amd/csrc/peaq_replay.hip).  The replay kernels serve 2 (basic) or
8 (advanced) spans of the list per wave, a lane picking its span by its slot in the wave; nine spans leave the basic
kernel a wave with an idle slot and the advanced ones a wave with one slot used.  The same nine spans are run as given,
reversed, and one at a time: every span's 16 doubles must be the same bytes in all three placements.
Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

import cases as case_defs
from test_gpu_windows import raw, to_device

pytestmark = pytest.mark.gpu

N = 100000
SPANS = ((0, 100000), (0, 30000), (12000, 24000), (24000, 24000), (50000, 3000), (65000, 1500), (3000, 1000),
         (90000, 20000),                               # runs past the end
         (100000, 5000))                               # begins at the end: no units


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("advanced", (0, 1))
def test_a_spans_reading_does_not_depend_on_its_place_in_the_list(gpu, advanced, channels):
    import gstpeaq_amd
    import torch
    r, t = case_defs.make_inputs(dict(kind="synth", seed=31, channels=channels, n=N, test_trim=1500))
    ref, test, n_ref, n_test = to_device([(r, t)])
    ctx = gpu.ctx("default")
    entry = gstpeaq_amd.batch_adv_spans if advanced else gstpeaq_amd.batch_windows

    def run(spans):
        rows, res = entry(ctx, ref, test, np.array(spans, dtype=np.uint32), n_ref, n_test, sync=False)
        torch.cuda.synchronize()
        rows, res = raw(rows), raw(res)
        assert rows.shape == (1, len(spans), 16) and res.shape == (1, 16)
        return rows[0], res[0].tobytes()

    plain = gstpeaq_amd.batch_run(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    plain = raw(plain)[0].tobytes()

    as_given, res = run(SPANS)
    assert res == plain
    backwards, res = run(SPANS[::-1])
    assert res == plain
    empty = full = 0
    for k, (start, length) in enumerate(SPANS):
        alone, res = run([(start, length)])
        assert res == plain, k
        print(advanced, channels, k, (start, length), as_given[k])
        assert as_given[k].tobytes() == alone[0].tobytes(), (k, as_given[k], alone[0])
        assert backwards[len(SPANS) - 1 - k].tobytes() == alone[0].tobytes(), (k, backwards[len(SPANS) - 1 - k], alone[0])
        frames = gstpeaq_amd.window_frames(len(r), len(t), start, length)[1]
        blocks = gstpeaq_amd.span_blocks(len(r), len(t), start, length)[1] if advanced else 0
        assert as_given[k][14] == frames and as_given[k][15] == blocks, (k, as_given[k][14:], frames, blocks)
        empty += frames == 0 and blocks == 0
        full += not np.isnan(as_given[k][:5 if advanced else 11]).any()
    assert as_given[0].tobytes() == plain              # (the span over the whole pair is the end result)
    assert empty >= 1 and full >= 1, (empty, full)
