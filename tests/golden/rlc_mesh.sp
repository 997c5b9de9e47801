V1 a 0 PULSE(0 1 2e-9 1e-9 1e-9 5e-9 20e-9)
I1 0 c PWL(0 0 5e-9 1e-3 30e-9 -1e-3)
R1 a b 50
L1 b c 2e-9
C1 c 0 1e-12
R2 c d 75
L2 d e 5e-9
C2 e 0 2e-12
R3 e 0 1e3
R4 b e 220
C3 b d 0.5e-12
V2 f 0 SIN 0.5 0.25 2e8 0
R5 f d 330
.TRAN 1e-10 8e-9
