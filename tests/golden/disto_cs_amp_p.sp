* common-source amplifier with source degeneration: HD2 and HD3 at the drain, PMOS (the mirror image of disto_cs_amp.sp)
VDD vdd 0 DC -3
VIN g 0 DC -1.2 AC 1m
RD vdd d 2k
RS s 0 200
CL d 0 1p
M1 d g s p 10e-6 1e-6 1
.MODEL 1 VT -0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.disto v(d) dec 5 1k 1g
