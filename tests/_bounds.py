"""The project's predict parity bounds, shared by GPU and CPU tests: against the reference's vectors, MAE < 1e-4 pA and max < 2e-3 pA."""
MAE_TOL, MAX_TOL = 1e-4, 2e-3
