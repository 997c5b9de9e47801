* common-source amplifier: AC gain against a small-signal transient
VDD vdd 0 DC 3
VIN g 0 DC 0 AC 1 SIN 0.9 10m 1meg 0
RD vdd d 5k
CL d 0 1p
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.TRAN 1e-10 3e-6
.AC DEC 10 1k 1g
