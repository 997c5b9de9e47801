* RC low-pass, tau = 200 periods of the 1 MHz tone
V1 in 0 SIN 0 100 1e6 0
R1 in out 1k
C1 out 0 200n
.TRAN 31.25n 1u
.hb 1e6 3
