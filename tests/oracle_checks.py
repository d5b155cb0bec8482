"""Elementwise check shared by the float64-oracle GPU tests."""

import torch


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; a zero bound demands equality."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    return float(ratio.max())


def assert_within(got, ref, bound, what):
    """Every element: |got - ref| <= bound. Non-finite values fail."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    excess = (got - ref).abs() - bound
    worst = int(excess.argmax())
    assert float(excess.flatten()[worst]) <= 0.0, (
        f"{what}: element {worst} got {float(got.flatten()[worst])!r} "
        f"ref {float(ref.flatten()[worst])!r} bound {float(bound.flatten()[worst])!r}")
