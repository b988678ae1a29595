"""mtsh_path_job_cancel counts from the entry of mtsh_path_job_render
(include/mtsg_path.h: "cancel the job's running render"): a cancel that arrives
while the call still cuts the tile shares and allocates the GPUs' blocks, before
its GPU threads start, must end the call with MTSG_ERR_CANCELLED instead of
being wiped as a cancel while idle.  The window is a few milliseconds for a
real frame; the test makes it long with a 10000 x 10000 rectangle (390,625
tiles to deal, a 2-GB block to allocate), which no GPU is ever asked to render:
the worker sees the job's flag first.  Without the cancel the same call
fails in the device library (the rectangle lies outside the 64 x 48 film)."""
import threading
import time

import pytest

import mtsg

pytestmark = pytest.mark.gpu


def test_cancel_before_the_gpu_threads_start_is_kept(cbox_small):
    job = mtsg.PathJob(cbox_small, 1)
    b = cbox_small.border
    huge = cbox_small.params(tile_w=10000, tile_h=10000, spp=1)
    entered = threading.Event()
    result = {}

    def work():
        entered.set()
        result["rc"], _, result["secs"] = job.render(huge, b)
        result["t_return"] = time.time()

    try:
        th = threading.Thread(target=work)
        th.start()
        assert entered.wait(10)
        time.sleep(0.1)   # inside the call by now, and seconds before its GPU threads
        t_cancel = time.time()
        job.cancel()
        th.join(120)
        assert not th.is_alive()
        print(f"cancel sent {result['t_return'] - t_cancel:.3f} s before the call returned")
        assert result["rc"] == mtsg.MTSG_ERR_CANCELLED, (result, job.last_error())
        # the cancel was consumed: the job's next render completes ...
        rc, img, _ = job.render(cbox_small.params(), b)
        assert rc == 0 and img[..., 4].sum() > 0, job.last_error()
        # ... and without a cancel the huge rectangle is the device library's error
        rc, _, _ = job.render(huge, b)
        assert rc not in (0, mtsg.MTSG_ERR_CANCELLED), rc
    finally:
        job.close()
