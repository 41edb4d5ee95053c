"""Self-check of the guarded buffers of tests/test_gpu_render_contract.py, on host memory: a write outside the payload must be reported.
(That module is marked gpu as a whole, so its one test that needs no GPU lives here.)"""
import pytest

from test_gpu_render_contract import FILL, GUARD, Guarded

torch = pytest.importorskip("torch")


def test_a_write_into_a_guard_is_reported():
    for delta in (0, 3, 1008):
        g = Guarded(1000, delta, device="cpu")
        assert (g.addr - delta) % 4096 == 0 and g.payload().data_ptr() == g.addr and g.payload().numel() == 1000
        g.check_guards("fresh"), g.check_untouched("fresh")
        g.payload().fill_(1)  # the payload is the caller's to write
        g.check_guards("payload written")
        with pytest.raises(AssertionError, match="was not passed"):
            g.check_untouched("payload written")
        # one byte each: just before and just behind the payload, the far ends of both guards, the first byte of the pointer's slack
        for at in {-1, 1000, -GUARD - delta, 1000 + GUARD - 1, -delta or -1}:
            h = Guarded(1000, delta, device="cpu")
            h.t[h.off + at] = FILL ^ 1
            assert h.touched() == [at], (delta, at)
            with pytest.raises(AssertionError, match="outside the caller's buffer"):
                h.check_guards(f"byte {at}")
            with pytest.raises(AssertionError, match="outside the caller's buffer"):
                h.check_untouched(f"byte {at}")
