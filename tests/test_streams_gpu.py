"""The stream hand-off helpers of spmm_amd/streams.py (`after`, `mark`): work on the waiting stream sees what the other stream had enqueued.
Two fresh streams, not the pool's: the suite's queue placement stays as it is."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 8_000_000          # torch.cuda._sleep counts device clocks (~2 GHz): a few milliseconds


@pytest.mark.parametrize("form", ["after", "mark"])
def test_handoff_orders_the_waiting_stream_behind_the_other(form):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import streams
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    src = torch.zeros(1024, device="cuda")
    dst = torch.zeros(1024, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        torch.cuda._sleep(SLEEP_CYCLES)                 # without the hand-off the copy below would run first and read zeros
        src.fill_(1.0)
    if form == "after":
        streams.after(b, a)
    else:
        ev = streams.mark(a)
        b.wait_event(ev)
    with torch.cuda.stream(b):
        dst.copy_(src)
    torch.cuda.synchronize()
    assert bool((dst == 1.0).all())
