"""What the context's status message says about the bits the batched matchers set: each bit's general description (kStatusText, csrc/olf_internal.hpp),
which names no entry point -- several entries set every one of these bits, so a message that named one would send a caller of another to the wrong call."""

STATUS_TEXT = {
    256: "a batched matcher left out a pair or a candidate that holds an octave outside the context's levels",
    512: "a batched point entry left out a list index or a per-frame map-point index outside the map",
    1024: "a batched line entry left out a list index or a per-frame map-line index outside the map",
    2048: "a pair entry skipped a pair whose frame indices are outside the batch or equal",
}


def describes(message, *bits):
    """True when `message` explains every one of `bits` by its general description"""
    return all("%d: %s" % (b, STATUS_TEXT[b]) in str(message) for b in bits)
