"""Training-side modules mirroring tfpnp/trainer (the value network; the MDDPG loop itself is not part of the package)."""
