"""Delay-Doppler models of the nadir_sar_altimetry solver (counterpart of smrt/rtsolver/delay_doppler_model)."""
